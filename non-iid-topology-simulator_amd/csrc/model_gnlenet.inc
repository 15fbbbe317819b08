// GN-LeNet on listed slab rows: evaluation (k_gnl_eval) and training (k_gnl_grad_sample,
// k_gnl_grad_conv, k_gnl_grad_fc).  Included by niidmix.hip after its linear-model section, on which
// it relies (lin_len, ev_len; its entry points also launch k_lin_eval_sum).
// ----------------------------------------------------------------------------------------------
// Evaluation of GN-LeNet (niidmix_gnlenet_eval_rows_f32; the reference's setup/model/gn_lenet.py):
//   conv1(Cin -> 32, 5 x 5, pad 2) -> maxpool(3, 2) -> GroupNorm(2) -> ReLU
//   conv2(32 -> 32) -> GroupNorm(2) -> maxpool(3, 2) -> ReLU
//   conv3(32 -> 64) -> GroupNorm(2) -> maxpool(3, 2) -> ReLU -> flatten -> linear(F -> C)
// k_gnl_eval: one workgroup per (job, tile of kGnTS samples) walks the whole network; a sample is
// never split over workgroups (the group statistics need its whole map).  Two activation buffers
// of kGnTS * 32 h1 w1 floats (the pooled conv1 map, the largest one kept) ping-pong through the
// layers: in LDS when they fit (up to 34 x 34 inputs), else in a slot of the scratch buffer owned
// by the workgroup (a persistent grid of at most kGnMaxSlots workgroups).
//   conv1     a lane per (sample, 8 output channels, pooled position): the 3 x 3 conv outputs
//             under the pool window from a 7 x 7 input patch in registers, pooled while written (the
//             full-resolution map, 98 KiB per MNIST sample, never exists).
//   conv2/3   implicit GEMM, K = 800: a lane per (sample, 8 output channels, row, 4 columns), 32
//             accumulators; the weights pass through LDS in stages of 6400 floats as [k][channel]
//             (float4 broadcast reads), the next stage's global loads in flight while the current
//             one is multiplied.  A job's 322 KB of weights are re-read by its tiles from L2.
//   GroupNorm a wave per (sample, group): the mean, then the centred squares, both fp32, lanes
//             striding the group's contiguous map, a fixed xor butterfly across the wave.
//   linear    a wave per class, lanes striding F, the same butterfly; softmax, argmax and loss as
//             k_lin_eval (ev_scan); partial sums per (job, tile), added by k_lin_eval_sum.
// Every value is a fixed-order chain of one workgroup: a job's bits depend on nothing but its row,
// its samples and the tile's position in the job.
constexpr int kGnTS = 2;                // samples per tile
constexpr int kGnOT = 8;                // output channels per lane
constexpr int kGnPX = 4;                // columns per lane (conv2, conv3)
constexpr int kGnStage = 6400;          // weights per stage: 8 input channels x 25 x 32, 4 x 25 x 64
constexpr int kGnWFloats = 7200;        // the stage in LDS, rows padded by 4: 200 x 36 >= 100 x 68
constexpr int kGnStat = 16 + 2 * kGnTS * 64;   // mean / rstd, nll / hit, then (scale, shift)
constexpr int kGnMaxCin = 4, kGnMinHW = 15, kGnMaxHW = 64;
constexpr int64_t kGnLdsMax = 160 * 1024;
constexpr int64_t kGnMaxSlots = 4096;
constexpr int64_t kGnMaxGrid = 1 << 20;

struct GnShape {
    int Cin, H, W, C;
    int h1, w1, h2, w2, h3, w3, F;
    // offsets of the 14 tensors in a row (model.parameters() order)
    int c1w, c1b, g1w, g1b, c2w, c2b, g2w, g2b, c3w, c3b, g3w, g3b, fw, fb;
    int64_t P;
};

__host__ __device__ inline int gn_down(int h) { return (h - 3) / 2 + 1; }

inline GnShape gn_shape(int Cin, int H, int W, int C) {
    GnShape g;
    g.Cin = Cin; g.H = H; g.W = W; g.C = C;
    g.h1 = gn_down(H); g.w1 = gn_down(W);
    g.h2 = gn_down(g.h1); g.w2 = gn_down(g.w1);
    g.h3 = gn_down(g.h2); g.w3 = gn_down(g.w2);
    g.F = 64 * g.h3 * g.w3;
    int o = 0;
    g.c1w = o; o += 32 * Cin * 25; g.c1b = o; o += 32; g.g1w = o; o += 32; g.g1b = o; o += 32;
    g.c2w = o; o += 32 * 32 * 25; g.c2b = o; o += 32; g.g2w = o; o += 32; g.g2b = o; o += 32;
    g.c3w = o; o += 64 * 32 * 25; g.c3b = o; o += 64; g.g3w = o; o += 64; g.g3b = o; o += 64;
    g.fw = o;
    g.fb = o + C * g.F;                           // C <= 1024, F <= 3136
    g.P = (int64_t)g.fb + C;
    return g;
}

// floats of one workgroup's two activation buffers
inline int64_t gn_act_floats(const GnShape &g) { return 2 * (int64_t)kGnTS * 32 * g.h1 * g.w1; }
inline int64_t gn_lds_bytes_global() { return (int64_t)(kGnWFloats + kGnStat) * 4; }
inline int64_t gn_lds_bytes(const GnShape &g) { return gn_lds_bytes_global() + gn_act_floats(g) * 4; }

// max_pool2d's maximum: a NaN wins and stays
__device__ __forceinline__ float gn_max(float a, float b) { return (b > a || b != b) ? b : a; }
__device__ __forceinline__ float gn_relu(float v) { return v <= 0.f ? 0.f : v; }

__device__ __forceinline__ float gn_wave_sum(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// conv1 + maxpool: in = the tile's samples [Cin, H, W] in global memory (sample s at xof(s), which
// clamps s to the tile), out [kGnTS, 32, h1, w1] = max over the 3 x 3 window of the conv outputs,
// plus the bias.  AM: amax [kGnTS, 32, h1, w1] gets the window position (3 row + column) of that
// maximum, the first one in scan order (gn_max's rule).
template <bool AM = false, class XOf>
__device__ __forceinline__ void gn_conv1_pool(XOf xof, const GnShape &g, const float *__restrict__ th,
                                              float *out, float *ws, unsigned char *amax = nullptr) {
    constexpr int WS = 32 + 4;
    const int tid = threadIdx.x;
    const int nk = g.Cin * 25;
    for (int e = tid; e < 32 * nk; e += 256) ws[(e % nk) * WS + e / nk] = th[g.c1w + e];
    __syncthreads();
    const int hw1 = g.h1 * g.w1, per_g = kGnTS * hw1;
#pragma unroll 1
    for (int item = tid; item < 4 * per_g; item += 256) {
        const int ocg = item / per_g, rem = item % per_g;
        const int s = rem / hw1, pos = rem % hw1;
        const int pi = pos / g.w1, pj = pos % g.w1;
        const float *xs = xof(s);
        float acc[9][kGnOT];
#pragma unroll
        for (int a = 0; a < 9; ++a)
#pragma unroll
            for (int o = 0; o < kGnOT; ++o) acc[a][o] = 0.f;
#pragma unroll 1
        for (int ic = 0; ic < g.Cin; ++ic) {
            float patch[7][7];
#pragma unroll
            for (int r = 0; r < 7; ++r) {
                const int yy = 2 * pi - 2 + r;
                const bool rok = (unsigned)yy < (unsigned)g.H;
#pragma unroll
                for (int c = 0; c < 7; ++c) {
                    const int xx = 2 * pj - 2 + c;
                    const bool ok = rok && (unsigned)xx < (unsigned)g.W;
                    const float v = xs[((int64_t)ic * g.H + (ok ? yy : 0)) * g.W + (ok ? xx : 0)];
                    patch[r][c] = ok ? v : 0.f;
                }
            }
#pragma unroll
            for (int ky = 0; ky < 5; ++ky)
#pragma unroll
                for (int kx = 0; kx < 5; ++kx) {
                    const float *wp = ws + (ic * 25 + ky * 5 + kx) * WS + ocg * kGnOT;
                    const float4 wa = *reinterpret_cast<const float4 *>(wp);
                    const float4 wb = *reinterpret_cast<const float4 *>(wp + 4);
                    const float wv[kGnOT] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w};
#pragma unroll
                    for (int di = 0; di < 3; ++di)
#pragma unroll
                        for (int dj = 0; dj < 3; ++dj)
#pragma unroll
                            for (int o = 0; o < kGnOT; ++o)
                                acc[di * 3 + dj][o] = __builtin_fmaf(patch[di + ky][dj + kx], wv[o], acc[di * 3 + dj][o]);
                }
        }
#pragma unroll
        for (int o = 0; o < kGnOT; ++o) {
            float m = acc[0][o];
            int am = 0;
#pragma unroll
            for (int a = 1; a < 9; ++a) {
                if (AM && (acc[a][o] > m || acc[a][o] != acc[a][o])) am = a;
                m = gn_max(m, acc[a][o]);
            }
            const int oc = ocg * kGnOT + o;
            out[(s * 32 + oc) * hw1 + pos] = m + th[g.c1b + oc];
            if constexpr (AM) amax[(s * 32 + oc) * hw1 + pos] = (unsigned char)am;
        }
    }
    __syncthreads();
}

// 5 x 5 convolution, CI -> CO channels, zero padding 2: in [kGnTS, CI, h, w] -> out [kGnTS, CO, h, w]
// (bias added).  wg: the weights [CO, CI, 5, 5] of the job's row, bg the bias.  Every output is
// one fma chain over (input channel, ky, kx) from 0.
// TR: the data gradient of such a convolution instead, a convolution with the flipped, transposed
// weights: wg is the forward weight [CI, CO, 5, 5], tap k of (output o, input c) is
// wg[c][o][24 - k], and there is no bias (bg is not read).
template <int CO, int CI = 32, bool TR = false>
__device__ __forceinline__ void gn_conv(const float *in, float *out, int h, int w,
                                        const float *__restrict__ wg, const float *__restrict__ bg,
                                        float *ws) {
    constexpr int ICB = kGnStage / (25 * CO);    // input channels per stage: 8 or 4
    constexpr int KR = ICB * 25;                 // k rows per stage
    constexpr int WS = CO + 4;
    constexpr int NST = CI / ICB;
    constexpr int NPRE = kGnStage / 256;
    static_assert(KR * WS <= kGnWFloats && NPRE * 256 == kGnStage, "stage size");
    const int tid = threadIdx.x;
    const int xg = (w + kGnPX - 1) / kGnPX, per_s = h * xg;
    const int n_items = (CO / kGnOT) * kGnTS * per_s;
#pragma unroll 1
    for (int base = 0; base < n_items; base += 512) {
        int is[2], iy[2], ix[2], io[2];
        bool ok[2];
        float acc[2][kGnPX][kGnOT];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int item = base + r * 256 + tid;
            ok[r] = item < n_items;
            const int it = ok[r] ? item : 0;
            io[r] = it / (kGnTS * per_s);
            const int rem = it % (kGnTS * per_s);
            is[r] = rem / per_s;
            iy[r] = (rem % per_s) / xg;
            ix[r] = ((rem % per_s) % xg) * kGnPX;
#pragma unroll
            for (int p = 0; p < kGnPX; ++p)
#pragma unroll
                for (int o = 0; o < kGnOT; ++o) acc[r][p][o] = 0.f;
        }
        float pre[NPRE];
        auto fetch = [&](int st) {               // element e of the stage: channel e / KR, k row e % KR
#pragma unroll
            for (int q = 0; q < NPRE; ++q) {
                const int e = q * 256 + tid;
                if constexpr (TR) pre[q] = wg[((st * ICB + (e % KR) / 25) * CO + e / KR) * 25 + 24 - (e % KR) % 25];
                else pre[q] = wg[((e / KR) * CI + st * ICB) * 25 + e % KR];
            }
        };
        fetch(0);
#pragma unroll 1
        for (int st = 0; st < NST; ++st) {
            __syncthreads();                     // the previous stage has been read
#pragma unroll
            for (int q = 0; q < NPRE; ++q) {
                const int e = q * 256 + tid;
                ws[(e % KR) * WS + e / KR] = pre[q];
            }
            __syncthreads();
            if (st + 1 < NST) fetch(st + 1);
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                if (base + r * 256 >= n_items) continue;          // block-uniform
#pragma unroll 1
                for (int icl = 0; icl < ICB; ++icl) {
                    const float *ip = in + ((is[r] * CI + st * ICB + icl) * h) * w;
#pragma unroll
                    for (int ky = 0; ky < 5; ++ky) {
                        const int yy = iy[r] + ky - 2;
                        const bool rok = (unsigned)yy < (unsigned)h;
                        const float *rp = ip + (rok ? yy : 0) * w;
                        float v[kGnPX + 4];
#pragma unroll
                        for (int e = 0; e < kGnPX + 4; ++e) {
                            const int xx = ix[r] - 2 + e;
                            const bool in_x = rok && (unsigned)xx < (unsigned)w;
                            const float t = rp[in_x ? xx : 0];
                            v[e] = in_x ? t : 0.f;
                        }
#pragma unroll
                        for (int kx = 0; kx < 5; ++kx) {
                            const float *wp = ws + (icl * 25 + ky * 5 + kx) * WS + io[r] * kGnOT;
                            const float4 wa = *reinterpret_cast<const float4 *>(wp);
                            const float4 wb = *reinterpret_cast<const float4 *>(wp + 4);
                            const float wv[kGnOT] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w};
#pragma unroll
                            for (int p = 0; p < kGnPX; ++p)
#pragma unroll
                                for (int o = 0; o < kGnOT; ++o)
                                    acc[r][p][o] = __builtin_fmaf(v[p + kx], wv[o], acc[r][p][o]);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (!ok[r]) continue;
#pragma unroll
            for (int o = 0; o < kGnOT; ++o) {
                const int oc = io[r] * kGnOT + o;
                float b = 0.f;
                if constexpr (!TR) b = bg[oc];
#pragma unroll
                for (int p = 0; p < kGnPX; ++p)
                    if (ix[r] + p < w)
                        out[((is[r] * CO + oc) * h + iy[r]) * w + ix[r] + p] = TR ? acc[r][p][o] : acc[r][p][o] + b;
            }
        }
    }
    __syncthreads();
}

// GroupNorm(2, CO) statistics of buf [kGnTS, CO, hw] in two passes, then per (sample, channel)
// scale = rstd * weight, shift = bias - scale * mean into stat[16 + 2 (s CO + c)].
template <int CO>
__device__ __forceinline__ void gn_stats(const float *buf, int hw, const float *__restrict__ gw,
                                         const float *__restrict__ gb, float *stat) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int n = (CO / 2) * hw;
    for (int pair = wave; pair < kGnTS * 2; pair += 4) {
        const float *p = buf + pair * n;         // (sample, group) maps are contiguous, in this order
        float a = 0.f;
        for (int i = lane; i < n; i += 64) a += p[i];
        const float mean = gn_wave_sum(a) / (float)n;
        float q = 0.f;
        for (int i = lane; i < n; i += 64) {
            const float d = p[i] - mean;
            q = __builtin_fmaf(d, d, q);
        }
        const float var = gn_wave_sum(q) / (float)n;
        if (lane == 0) {
            stat[pair * 2] = mean;
            stat[pair * 2 + 1] = 1.0f / sqrtf(var + 1e-5f);
        }
    }
    __syncthreads();
    for (int e = tid; e < kGnTS * CO; e += 256) {
        const int c = e % CO, pair = (e / CO) * 2 + c / (CO / 2);
        const float scale = stat[pair * 2 + 1] * gw[c];
        stat[16 + 2 * e] = scale;
        stat[16 + 2 * e + 1] = __builtin_fmaf(-scale, stat[pair * 2], gb[c]);
    }
    __syncthreads();
}

// out [kGnTS, CO, ho, wo] = relu(maxpool(3, 2)(in * scale + shift)), in [kGnTS, CO, h, w]
template <int CO>
__device__ __forceinline__ void gn_norm_pool(const float *in, float *out, int h, int w, int ho, int wo,
                                             const float *stat) {
    for (int e = threadIdx.x; e < kGnTS * CO * ho * wo; e += 256) {
        const int j = e % wo, i = (e / wo) % ho, sc = e / (wo * ho);
        const float scale = stat[16 + 2 * sc], shift = stat[16 + 2 * sc + 1];
        const float *p = in + (sc * h + 2 * i) * w + 2 * j;
        float m = __builtin_fmaf(p[0], scale, shift);
#pragma unroll
        for (int a = 1; a < 9; ++a) m = gn_max(m, __builtin_fmaf(p[(a / 3) * w + a % 3], scale, shift));
        out[e] = gn_relu(m);
    }
    __syncthreads();
}

// classifier: feat is [kGnTS, F] in (channel, row, column) order; logits to z [kGnTS, C]
__device__ __forceinline__ void gn_linear(const float *feat, const GnShape &g, const float *__restrict__ th,
                                          float *zout) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int c = wave; c < g.C; c += 4) {
        const float *wr = th + g.fw + (int64_t)c * g.F;
        float z[kGnTS];
#pragma unroll
        for (int s = 0; s < kGnTS; ++s) z[s] = 0.f;
        for (int f = lane; f < g.F; f += 64) {
            const float wv = wr[f];
#pragma unroll
            for (int s = 0; s < kGnTS; ++s) z[s] = __builtin_fmaf(feat[s * g.F + f], wv, z[s]);
        }
        const float b = th[g.fb + c];
#pragma unroll
        for (int s = 0; s < kGnTS; ++s) {
            const float v = gn_wave_sum(z[s]) + b;
            if (lane == 0) zout[s * g.C + c] = v;
        }
    }
    __syncthreads();
}

template <bool LDS>
__global__ __launch_bounds__(256) void k_gnl_eval(const float *__restrict__ theta, int64_t ld_t,
                                                  const float *__restrict__ data,
                                                  const int32_t *__restrict__ labels,
                                                  const int32_t *__restrict__ rows,
                                                  const int32_t *__restrict__ seg_start,
                                                  const int32_t *__restrict__ seg_len, int64_t n_jobs,
                                                  int max_len, int n_tiles, const GnShape g,
                                                  double *__restrict__ part_loss,
                                                  int32_t *__restrict__ part_cnt,
                                                  int32_t *__restrict__ pred, int64_t ld_pred,
                                                  float *__restrict__ logits, int64_t ld_logits,
                                                  float *act) {
    extern __shared__ __attribute__((aligned(16))) float gn_smem[];
    float *ws = gn_smem, *stat = gn_smem + kGnWFloats;
    const int tid = threadIdx.x;
    const int hw1 = g.h1 * g.w1, a1 = kGnTS * 32 * hw1;
    float *buf_a, *buf_b;
    if constexpr (LDS) buf_a = gn_smem + kGnWFloats + kGnStat;
    else buf_a = act + (int64_t)blockIdx.x * (2 * a1);
    buf_b = buf_a + a1;
    const int64_t n_work = n_jobs * n_tiles, sample = (int64_t)g.Cin * g.H * g.W;
    for (int64_t wk = blockIdx.x; wk < n_work; wk += gridDim.x) {       // wk = job * n_tiles + tile
        const int64_t job = wk / n_tiles;
        const int t = (int)(wk % n_tiles);
        const int left = ev_len(seg_len, job, max_len) - t * kGnTS;
        if (left <= 0) continue;                                      // block-uniform
        const int ns = left < kGnTS ? left : kGnTS;
        const int64_t s0 = (int64_t)seg_start[job] + (int64_t)t * kGnTS;
        const float *th = theta + (int64_t)rows[job] * ld_t;

        const float *x0 = data + s0 * sample;
        gn_conv1_pool([&](int s) { return x0 + (int64_t)(s < ns ? s : 0) * sample; }, g, th, buf_a, ws);
        gn_stats<32>(buf_a, hw1, th + g.g1w, th + g.g1b, stat);
        for (int e = tid; e < a1; e += 256)
            buf_a[e] = gn_relu(__builtin_fmaf(buf_a[e], stat[16 + 2 * (e / hw1)], stat[16 + 2 * (e / hw1) + 1]));
        __syncthreads();
        gn_conv<32>(buf_a, buf_b, g.h1, g.w1, th + g.c2w, th + g.c2b, ws);
        gn_stats<32>(buf_b, hw1, th + g.g2w, th + g.g2b, stat);
        gn_norm_pool<32>(buf_b, buf_a, g.h1, g.w1, g.h2, g.w2, stat);
        gn_conv<64>(buf_a, buf_b, g.h2, g.w2, th + g.c3w, th + g.c3b, ws);
        gn_stats<64>(buf_b, g.h2 * g.w2, th + g.g3w, th + g.g3b, stat);
        gn_norm_pool<64>(buf_b, buf_a, g.h2, g.w2, g.h3, g.w3, stat);

        gn_linear(buf_a, g, th, ws);
        if (logits)
            for (int e = tid; e < ns * g.C; e += 256)
                logits[(job * ld_logits + (int64_t)t * kGnTS) * g.C + e] = ws[e];
        if (tid < ns) {
            const int y = labels[s0 + tid];
            EvState q;
            ev_scan(ws + tid * g.C, g.C, 0, y, true, q);
            stat[8 + tid] = (q.best + logf(q.sum)) - q.zy;
            stat[8 + kGnTS + tid] = q.idx == y ? 1.f : 0.f;
            if (pred) pred[job * ld_pred + (int64_t)t * kGnTS + tid] = q.idx;
        }
        __syncthreads();
        if (tid == 0) {                                               // in sample order
            double a = 0.0;
            int c = 0;
            for (int s = 0; s < ns; ++s) {
                a += (double)stat[8 + s];
                c += stat[8 + kGnTS + s] != 0.f;
            }
            part_loss[wk] = a;
            part_cnt[wk] = c;
        }
        __syncthreads();                                              // ws, stat and the buffers are free
    }
}

// ----------------------------------------------------------------------------------------------
// Local training of GN-LeNet on listed rows (niidmix_gnlenet_nll_grad_rows_f32): the gradient of
// F.nll_loss(model.forward(x), y) on a zeroed gradient, the forward being k_gnl_eval's.
//   k_gnl_grad_sample   one workgroup per (row, tile of kGnTS samples).  The forward functions above
//                       run on the batch's gathered samples with every activation buffer in the
//                       tile's scratch slot (the backward needs them there in any case, so there is
//                       no LDS variant and no size-dependent path), then the sample-local backward
//                       chain: dz, the feature gradient, and per stage max-pool / ReLU, GroupNorm
//                       and the convolution's data gradient (gn_conv<.., TR>).  The pool's backward
//                       is a gather: a source position adds the output gradients of the at most 4
//                       windows that cover it and whose first maximum (gn_max's rule, recomputed
//                       from the same fmas as the forward) it is.  No atomics.
//   k_gnl_grad_conv     one workgroup per (row, convolution output channel): the weight gradient of
//                       its [CI, 5, 5] filter, the bias gradient and the channel's two GroupNorm
//                       gradients.  Per sample one fma chain over the <= h w positions, the samples
//                       then added in batch order.  conv1 reads the input at the argmax positions.
//   k_gnl_grad_fc       a lane per classifier weight: one fma chain over the samples in batch order;
//                       the bias; the mean loss.
// Every value is a fixed-order chain or tree of one workgroup over one row's own data.
struct GnGradLay {     // float offsets in a tile's scratch slot; every array is [kGnTS, ...]
    int p1, x2, y2, dy2, dx2;     // [32, h1, w1]: pooled conv1, conv2's input, conv2's output, gradients
    int x3, dx3, y3, dy3;         // [32, h2, w2] conv3's input, [64, h2, w2] its output, gradients
    int feat, dfeat;              // [F]
    int st1, st2, st3;            // gn_stats' stat array of each stage (kGnStat floats)
    int gp1, gp2, gp3;            // [CO, 2]: per-sample (dgamma, dbeta)
    int dz, nll;                  // [C], [1]
    int amax;                     // bytes [32, h1, w1]: the first pool's argmax
    int tile;                     // floats per slot
};

inline GnGradLay gn_grad_lay(const GnShape &g) {
    GnGradLay L;
    int o = 0;
    auto take = [&](int n) { const int r = o; o += (n + 3) / 4 * 4; return r; };
    const int a1 = kGnTS * 32 * g.h1 * g.w1, a2 = kGnTS * 32 * g.h2 * g.w2;
    L.p1 = take(a1); L.x2 = take(a1); L.y2 = take(a1); L.dy2 = take(a1); L.dx2 = take(a1);
    L.x3 = take(a2); L.dx3 = take(a2); L.y3 = take(2 * a2); L.dy3 = take(2 * a2);
    L.feat = take(kGnTS * g.F); L.dfeat = take(kGnTS * g.F);
    L.st1 = take(kGnStat); L.st2 = take(kGnStat); L.st3 = take(kGnStat);
    L.gp1 = take(kGnTS * 64); L.gp2 = take(kGnTS * 64); L.gp3 = take(kGnTS * 128);
    L.dz = take(kGnTS * g.C); L.nll = take(kGnTS);
    L.amax = take((a1 + 3) / 4);
    L.tile = o;                                   // < 2^19 floats at 64 x 64, C 1024
    return L;
}

// Backward of relu(maxpool(3, 2)(y * scale + shift)): dn [kGnTS, CO, h, w] = the gradient with
// respect to the normalised map, gathered per source position.  pooled is the forward's output
// (after ReLU), dout its gradient, st the stage's saved stat array.
template <int CO>
__device__ __forceinline__ void gn_pool_bwd(const float *y, const float *pooled, const float *dout,
                                            float *dn, int h, int w, int ho, int wo, const float *st) {
    for (int e = threadIdx.x; e < kGnTS * CO * h * w; e += 256) {
        const int x = e % w, yy = (e / w) % h, sc = e / (w * h);
        const float scale = st[16 + 2 * sc], shift = st[16 + 2 * sc + 1];
        const int i0 = yy < 2 ? 0 : (yy - 1) / 2, i1 = yy / 2 < ho - 1 ? yy / 2 : ho - 1;
        const int j0 = x < 2 ? 0 : (x - 1) / 2, j1 = x / 2 < wo - 1 ? x / 2 : wo - 1;
        float acc = 0.f;
        for (int i = i0; i <= i1; ++i)
            for (int j = j0; j <= j1; ++j) {
                if (pooled[(sc * ho + i) * wo + j] <= 0.f) continue;     // ReLU; a NaN passes
                const float *p = y + (sc * h + 2 * i) * w + 2 * j;
                float m = __builtin_fmaf(p[0], scale, shift);
                int am = 0;
#pragma unroll
                for (int a = 1; a < 9; ++a) {
                    const float v = __builtin_fmaf(p[(a / 3) * w + a % 3], scale, shift);
                    if (v > m || v != v) { m = v; am = a; }
                }
                if (am == (yy - 2 * i) * 3 + (x - 2 * j)) acc += dout[(sc * ho + i) * wo + j];
            }
        dn[e] = acc;
    }
    __syncthreads();
}

// Backward of GroupNorm(2, CO): dn [kGnTS, CO, hw] holds the gradient of the normalised map and
// receives that of the input y.  gp [kGnTS, CO, 2] gets the sample's (dgamma, dbeta); red: 4 kGnTS
// floats of LDS.  With xh = (y - mean) rstd, gh = dn gamma:
//   dy = rstd (gh - mean(gh) - xh mean(gh xh)), the means over the (sample, group).
template <int CO>
__device__ __forceinline__ void gn_norm_bwd(const float *y, float *dn, int hw,
                                            const float *__restrict__ gw, const float *st, float *gp,
                                            float *red) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int sc = wave; sc < kGnTS * CO; sc += 4) {       // a wave per (sample, channel)
        const int pair = (sc / CO) * 2 + (sc % CO) / (CO / 2);
        const float mean = st[pair * 2], rstd = st[pair * 2 + 1];
        float a = 0.f, b = 0.f;
        for (int i = lane; i < hw; i += 64) {
            const float d = dn[sc * hw + i];
            a += d;
            b = __builtin_fmaf(d, (y[sc * hw + i] - mean) * rstd, b);
        }
        a = gn_wave_sum(a);
        b = gn_wave_sum(b);
        if (lane == 0) { gp[2 * sc] = b; gp[2 * sc + 1] = a; }
    }
    __syncthreads();
    if (tid < kGnTS * 2) {                                // a lane per (sample, group)
        const int s = tid / 2, c0 = (tid % 2) * (CO / 2);
        float a = 0.f, b = 0.f;
        for (int c = c0; c < c0 + CO / 2; ++c) {
            a = __builtin_fmaf(gw[c], gp[2 * (s * CO + c) + 1], a);
            b = __builtin_fmaf(gw[c], gp[2 * (s * CO + c)], b);
        }
        const float n = (float)((CO / 2) * hw);
        red[2 * tid] = a / n;
        red[2 * tid + 1] = b / n;
    }
    __syncthreads();
    for (int e = tid; e < kGnTS * CO * hw; e += 256) {
        const int sc = e / hw, c = sc % CO, pair = (sc / CO) * 2 + c / (CO / 2);
        const float rstd = st[pair * 2 + 1];
        const float xh = (y[e] - st[pair * 2]) * rstd;
        dn[e] = rstd * ((dn[e] * gw[c] - red[2 * pair]) - xh * red[2 * pair + 1]);
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void k_gnl_grad_sample(const float *__restrict__ theta, int64_t ld_t,
                                                         const float *__restrict__ data,
                                                         const int32_t *__restrict__ labels,
                                                         const int32_t *__restrict__ batch_idx,
                                                         const int32_t *__restrict__ batch_len, int b_max,
                                                         const int32_t *__restrict__ rows, int64_t n_rows,
                                                         int n_tiles, const GnShape g, const GnGradLay L,
                                                         float *scratch) {
    extern __shared__ __attribute__((aligned(16))) float gn_smem[];
    __shared__ float lse[kGnTS];
    __shared__ int ys[kGnTS];
    float *ws = gn_smem, *stat = gn_smem + kGnWFloats;
    const int tid = threadIdx.x;
    const int hw1 = g.h1 * g.w1, hw2 = g.h2 * g.w2, a1 = kGnTS * 32 * hw1;
    const int64_t n_work = n_rows * n_tiles, sample = (int64_t)g.Cin * g.H * g.W;
    for (int64_t wk = blockIdx.x; wk < n_work; wk += gridDim.x) {       // wk = row entry * n_tiles + tile
        const int64_t i = wk / n_tiles;
        const int t = (int)(wk % n_tiles);
        const int len = lin_len(batch_len, i, b_max), left = len - t * kGnTS;
        if (left <= 0) continue;                                      // block-uniform
        const int ns = left < kGnTS ? left : kGnTS;
        const float *th = theta + (int64_t)rows[i] * ld_t;
        const int32_t *bi = batch_idx + i * b_max + t * kGnTS;
        float *T = scratch + wk * L.tile;
        auto save_stat = [&](int off) {
            for (int e = tid; e < kGnStat; e += 256) T[off + e] = stat[e];
        };

        // forward, every map kept
        gn_conv1_pool<true>([&](int s) { return data + (int64_t)bi[s < ns ? s : 0] * sample; }, g, th,
                            T + L.p1, ws, reinterpret_cast<unsigned char *>(T + L.amax));
        gn_stats<32>(T + L.p1, hw1, th + g.g1w, th + g.g1b, stat);
        save_stat(L.st1);
        for (int e = tid; e < a1; e += 256)
            T[L.x2 + e] = gn_relu(__builtin_fmaf(T[L.p1 + e], stat[16 + 2 * (e / hw1)], stat[16 + 2 * (e / hw1) + 1]));
        __syncthreads();
        gn_conv<32>(T + L.x2, T + L.y2, g.h1, g.w1, th + g.c2w, th + g.c2b, ws);
        gn_stats<32>(T + L.y2, hw1, th + g.g2w, th + g.g2b, stat);
        save_stat(L.st2);
        gn_norm_pool<32>(T + L.y2, T + L.x3, g.h1, g.w1, g.h2, g.w2, stat);
        gn_conv<64>(T + L.x3, T + L.y3, g.h2, g.w2, th + g.c3w, th + g.c3b, ws);
        gn_stats<64>(T + L.y3, hw2, th + g.g3w, th + g.g3b, stat);
        save_stat(L.st3);
        gn_norm_pool<64>(T + L.y3, T + L.feat, g.h2, g.w2, g.h3, g.w3, stat);
        gn_linear(T + L.feat, g, th, ws);

        // loss and dz = (softmax(z) - onehot(y)) / len; the tile's unused samples get 0
        if (tid < ns) {
            const int y = labels[bi[tid]];
            EvState q;
            ev_scan(ws + tid * g.C, g.C, 0, y, true, q);
            const float l = q.best + logf(q.sum);
            lse[tid] = l;
            ys[tid] = y;
            T[L.nll + tid] = l - q.zy;
        }
        __syncthreads();
        const float flen = (float)len;
        for (int e = tid; e < kGnTS * g.C; e += 256) {
            const int s = e / g.C, c = e % g.C;
            const float dz = s < ns ? (expf(ws[e] - lse[s]) - (c == ys[s] ? 1.f : 0.f)) / flen : 0.f;
            ws[e] = dz;
            T[L.dz + e] = dz;
        }
        __syncthreads();
        for (int e = tid; e < kGnTS * g.F; e += 256) {                // the feature gradient
            const int s = e / g.F, f = e % g.F;
            const float *wc = th + g.fw + f;
            float acc = 0.f;
            for (int c = 0; c < g.C; ++c) acc = __builtin_fmaf(ws[s * g.C + c], wc[(int64_t)c * g.F], acc);
            T[L.dfeat + e] = acc;
        }
        __syncthreads();

        gn_pool_bwd<64>(T + L.y3, T + L.feat, T + L.dfeat, T + L.dy3, g.h2, g.w2, g.h3, g.w3, T + L.st3);
        gn_norm_bwd<64>(T + L.y3, T + L.dy3, hw2, th + g.g3w, T + L.st3, T + L.gp3, stat);
        gn_conv<32, 64, true>(T + L.dy3, T + L.dx3, g.h2, g.w2, th + g.c3w, nullptr, ws);
        gn_pool_bwd<32>(T + L.y2, T + L.x3, T + L.dx3, T + L.dy2, g.h1, g.w1, g.h2, g.w2, T + L.st2);
        gn_norm_bwd<32>(T + L.y2, T + L.dy2, hw1, th + g.g2w, T + L.st2, T + L.gp2, stat);
        gn_conv<32, 32, true>(T + L.dy2, T + L.dx2, g.h1, g.w1, th + g.c2w, nullptr, ws);
        for (int e = tid; e < a1; e += 256)
            if (T[L.x2 + e] <= 0.f) T[L.dx2 + e] = 0.f;               // ReLU; a NaN passes
        __syncthreads();
        gn_norm_bwd<32>(T + L.p1, T + L.dx2, hw1, th + g.g1w, T + L.st1, T + L.gp1, stat);
    }
}

constexpr int kGnMaxHW1 = ((kGnMaxHW - 3) / 2 + 1) * ((kGnMaxHW - 3) / 2 + 1);     // 31 x 31

__global__ __launch_bounds__(256) void k_gnl_grad_conv(const float *__restrict__ data,
                                                       const int32_t *__restrict__ batch_idx,
                                                       const int32_t *__restrict__ batch_len, int b_max,
                                                       const int32_t *__restrict__ rows, int n_tiles,
                                                       const GnShape g, const GnGradLay L,
                                                       const float *__restrict__ scratch,
                                                       float *__restrict__ grad, int64_t ld_g) {
    __shared__ float dys[kGnMaxHW1];
    __shared__ unsigned char ams[kGnMaxHW1 + 3];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t i = blockIdx.x / 128;
    const int ch = (int)(blockIdx.x % 128);
    const int layer = ch < 32 ? 1 : ch < 64 ? 2 : 3;
    const int oc = layer == 1 ? ch : layer == 2 ? ch - 32 : ch - 64;
    const int CO = layer == 3 ? 64 : 32, CI = layer == 1 ? g.Cin : 32;
    const int h = layer == 3 ? g.h2 : g.h1, w = layer == 3 ? g.w2 : g.w1, hw = h * w;
    const int nel = CI * 25;
    const int o_dy = layer == 1 ? L.dx2 : layer == 2 ? L.dy2 : L.dy3;
    const int o_x = layer == 2 ? L.x2 : L.x3, o_gp = layer == 1 ? L.gp1 : layer == 2 ? L.gp2 : L.gp3;
    const int len = lin_len(batch_len, i, b_max);
    const int64_t sample = (int64_t)g.Cin * g.H * g.W;
    float tot[4] = {0.f, 0.f, 0.f, 0.f}, btot = 0.f;
    for (int s = 0; s < len; ++s) {                                   // the samples in batch order
        const float *T = scratch + (i * n_tiles + s / kGnTS) * L.tile;
        const int sl = s % kGnTS;
        __syncthreads();                                              // the last sample has been read
        for (int p = tid; p < hw; p += 256) {
            dys[p] = T[o_dy + (sl * CO + oc) * hw + p];
            if (layer == 1) ams[p] = reinterpret_cast<const unsigned char *>(T + L.amax)[(sl * 32 + oc) * hw + p];
        }
        __syncthreads();
        if (wave == 3) {                                              // the bias: lanes stride the map
            float a = 0.f;
            for (int p = lane; p < hw; p += 64) a += dys[p];
            btot += gn_wave_sum(a);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = tid + 256 * q;
            if (e >= nel) continue;
            const int ic = e / 25, ky = (e % 25) / 5, kx = e % 5;
            float acc = 0.f;
            if (layer == 1) {                                         // the input at the argmax positions
                const float *xin = data + (int64_t)batch_idx[i * b_max + s] * sample + (int64_t)ic * g.H * g.W;
                for (int p = 0; p < hw; ++p) {
                    const int a = ams[p];
                    const int yy = 2 * (p / w) + a / 3 + ky - 2, xx = 2 * (p % w) + a % 3 + kx - 2;
                    if ((unsigned)yy < (unsigned)g.H && (unsigned)xx < (unsigned)g.W)
                        acc = __builtin_fmaf(dys[p], xin[yy * g.W + xx], acc);
                }
            } else {
                const float *xin = T + o_x + (sl * 32 + ic) * hw;
                const int y0 = ky < 2 ? 2 - ky : 0, y1 = ky > 2 ? h + 2 - ky : h;
                const int x0 = kx < 2 ? 2 - kx : 0, x1 = kx > 2 ? w + 2 - kx : w;
                for (int y = y0; y < y1; ++y)
                    for (int x = x0; x < x1; ++x)
                        acc = __builtin_fmaf(dys[y * w + x], xin[(y + ky - 2) * w + x + kx - 2], acc);
            }
            tot[q] += acc;
        }
    }
    float *gr = grad + (int64_t)rows[i] * ld_g;
    const int o_w = layer == 1 ? g.c1w : layer == 2 ? g.c2w : g.c3w;
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (tid + 256 * q < nel) gr[o_w + oc * nel + tid + 256 * q] = tot[q];
    if (tid == 192) gr[o_w + CO * nel + oc] = btot;                   // the bias follows its weight
    if (tid == 0) {                                                   // GroupNorm's weight and bias
        float dg = 0.f, db = 0.f;
        for (int s = 0; s < len; ++s) {
            const float *gp = scratch + (i * n_tiles + s / kGnTS) * L.tile + o_gp + 2 * ((s % kGnTS) * CO + oc);
            dg += gp[0];
            db += gp[1];
        }
        gr[o_w + CO * nel + CO + oc] = dg;
        gr[o_w + CO * nel + 2 * CO + oc] = db;
    }
}

__global__ __launch_bounds__(256) void k_gnl_grad_fc(const int32_t *__restrict__ batch_len, int b_max,
                                                     const int32_t *__restrict__ rows, int n_tiles,
                                                     int n_blk, const GnShape g, const GnGradLay L,
                                                     const float *__restrict__ scratch,
                                                     float *__restrict__ grad, int64_t ld_g,
                                                     float *__restrict__ loss) {
    const int64_t i = blockIdx.x / n_blk;
    const int e = (int)(blockIdx.x % n_blk) * 256 + threadIdx.x;
    const int len = lin_len(batch_len, i, b_max), nw = g.C * g.F;
    const float *T0 = scratch + i * n_tiles * L.tile;
    float *gr = grad + (int64_t)rows[i] * ld_g;
    if (e < nw + g.C) {
        const int c = e < nw ? e / g.F : e - nw, f = e % g.F;
        float acc = 0.f;
        for (int s = 0; s < len; ++s) {
            const float *T = T0 + (int64_t)(s / kGnTS) * L.tile;
            const float dz = T[L.dz + (s % kGnTS) * g.C + c];
            acc = e < nw ? __builtin_fmaf(dz, T[L.feat + (s % kGnTS) * g.F + f], acc) : acc + dz;
        }
        gr[g.fw + e] = acc;
    }
    if (e == 0) {                                                     // the mean loss, in batch order
        float a = 0.f;
        for (int s = 0; s < len; ++s) a += T0[(int64_t)(s / kGnTS) * L.tile + L.nll + s % kGnTS];
        loss[i] = a / (float)len;
    }
}
