// GN-LeNet evaluation with conv2 / conv3 on the matrix cores (k_gnl_eval_mfma,
// niidmix_gnlenet_eval_rows_mfma_f32).  Included by niidmix.hip after model_gnlenet.inc, whose
// conv1, GroupNorm, pooling and classifier functions it instantiates at its own tile size.
// ----------------------------------------------------------------------------------------------
// Job model, outputs and contract are k_gnl_eval's: one workgroup per (job, tile of TS samples)
// walks the whole network.  conv2 (32 -> 32) and conv3 (32 -> 64) are implicit GEMMs on
// v_mfma_f32_32x32x2_f32:
//   M   the tile's output positions (sample, row, column) flattened over the TS samples, cut in
//       M-tiles of 32; wave w owns M-tiles w, w + 4, ... and keeps their accumulators in registers
//       for the whole K loop (at most kGnMfmaMT2 / kGnMfmaMT3 of them)
//   N   the output channels: one N-tile of 32 for conv2, two for conv3
//   K   800 = (input channel, tap), walked as (weight stage, channel pair, ky, kx); the two lane
//       halves of an MFMA take the pair's two channels at the same tap
//   A   read from the activation buffer in LDS, one ds_read_b32 per lane and MFMA, no bounds
//       branch: the input lives in a SHARED-HALO layout.  Channel sc = s * 32 + c starts at
//       sc * cp, cp = (h + 2)(w + 2), its rows have pitch w + 2, and pixel (y, x) is at
//       (y + 2) * pitch + x + 2.  Columns 0, 1 of every row and rows 0, 1 of every channel are
//       zero: a row's right halo is the next row's left one, a channel's bottom halo the next
//       channel's top one, and 2 * pitch + 2 zeros follow the last channel.  That is 225 floats
//       per 13 x 13 channel where a private halo of 2 takes 289, which is what lets 4 MNIST
//       samples share one workgroup.
//   B   gn_conv's weight stage: 6400 floats in LDS as [k][channel] with the next stage's global
//       loads in flight; a value is read once per wave and stage and used by all its M-tiles
//   D   after the last stage and a barrier, written (plus the bias) over the input buffer as the
//       compact [TS, CO, h, w] map that gn_stats and gn_norm_pool read: one buffer per layer
// Every output is one K-order chain that does not depend on its position in M, so a sample's bits
// do not depend on the tile position it takes either.
constexpr int kGnMfmaMT2 = 7, kGnMfmaMT3 = 2;    // M-tiles per wave at most: conv2, conv3

__host__ __device__ inline int gn_halo_cp(int h, int w) { return (h + 2) * (w + 2); }
__host__ __device__ inline int gn_halo_tail(int w) { return 2 * (w + 2) + 2; }
__host__ __device__ inline int gn_mfma_wave_tiles(int m) { return ((m + 31) / 32 + 3) / 4; }

// floats of a workgroup's one activation buffer at ts samples per tile: the largest of conv2's
// halo'd input; conv2's compact output with conv3's halo'd input behind it; conv3's compact
// output with the features behind it
inline int64_t gn_mfma_act_floats(const GnShape &g, int ts) {
    const int64_t hw1 = g.h1 * g.w1, hw2 = g.h2 * g.w2;
    const int64_t in2 = ts * 32 * (int64_t)gn_halo_cp(g.h1, g.w1) + gn_halo_tail(g.w1);
    const int64_t in3 = ts * 32 * (hw1 + gn_halo_cp(g.h2, g.w2)) + gn_halo_tail(g.w2);
    const int64_t fc = ts * (64 * hw2 + g.F);
    return in2 > in3 ? (in2 > fc ? in2 : fc) : (in3 > fc ? in3 : fc);
}
inline int64_t gn_mfma_lds_bytes(const GnShape &g, int ts) {
    return (kGnWFloats + 16 + 2 * ts * 64 + gn_mfma_act_floats(g, ts)) * 4;
}
// THE rule for the samples per tile: the most of 4 and 2 whose weight stage, statistics and
// activation buffer fit kGnLdsMax and whose waves own at most kGnMfmaMT2 / kGnMfmaMT3 M-tiles;
// 0 when neither does (NIIDMIX_EUNSUPPORTED).  4 up to 13 x 13 pooled maps (28 x 28 inputs), 2 up
// to 20 x 20 (42 x 42); niidmix.ops.gn_mfma_tile restates it for the host.
inline int gn_mfma_ts(const GnShape &g) {
    for (int ts = 4; ts >= 2; ts -= 2)
        if (gn_mfma_lds_bytes(g, ts) <= kGnLdsMax && gn_mfma_wave_tiles(ts * g.h1 * g.w1) <= kGnMfmaMT2 &&
            gn_mfma_wave_tiles(ts * g.h2 * g.w2) <= kGnMfmaMT3)
            return ts;
    return 0;
}

// zeros of the shared-halo layout of nch channels of h x w at buf: rows 0 and 1 of every channel,
// columns 0 and 1 of every other row, the tail.  No barrier.
__device__ __forceinline__ void gn_halo_zero(float *buf, int nch, int h, int w) {
    const int pitch = w + 2;
    for (int it = threadIdx.x; it < nch * (h + 2); it += 256) {       // (channel, row): at it * pitch
        float *p = buf + it * pitch;
        const int n = it % (h + 2) < 2 ? pitch : 2;
        for (int c = 0; c < n; ++c) p[c] = 0.f;
    }
    for (int e = threadIdx.x; e < gn_halo_tail(w); e += 256) buf[nch * gn_halo_cp(h, w) + e] = 0.f;
}

// buf [NCH, h, w] compact (NCH = samples x channels) -> the shared-halo layout, in place; ACT: as
// relu(buf * scale + shift) on the way, else unchanged (a gradient map).  An element never moves
// down, so chunks of 2048 go from the top: read, barrier, write, barrier.
template <int NCH, bool ACT = true>
__device__ __forceinline__ void gn_halo_expand(float *buf, int h, int w, const float *stat) {
    constexpr int R = 8;
    const int hw = h * w, n = NCH * hw, pitch = w + 2, cp = gn_halo_cp(h, w);
#pragma unroll 1
    for (int top = n; top > 0; top -= 256 * R) {
        float v[R];
#pragma unroll
        for (int q = 0; q < R; ++q) {
            const int e = top - 1 - (q * 256 + (int)threadIdx.x);
            if (e >= 0) {
                if constexpr (ACT) v[q] = gn_relu(__builtin_fmaf(buf[e], stat[16 + 2 * (e / hw)], stat[16 + 2 * (e / hw) + 1]));
                else v[q] = buf[e];
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < R; ++q) {
            const int e = top - 1 - (q * 256 + (int)threadIdx.x);
            if (e >= 0) {
                const int sc = e / hw, pos = e % hw;
                buf[sc * cp + (pos / w + 2) * pitch + pos % w + 2] = v[q];
            }
        }
        __syncthreads();
    }
    gn_halo_zero(buf, NCH, h, w);
    __syncthreads();
}

// one weight stage of the K loop for a wave that owns MT M-tiles: per (channel pair, tap) the B
// value of each N-tile once, an A value per M-tile, MT * CO / 32 MFMAs
template <int CO, int MT, int MTMAX>
__device__ __forceinline__ void gn_mma_stage(floatx16 (&acc)[MTMAX][CO / 32], const float *in,
                                             const int (&ab)[MTMAX], const float *ws, int pitch, int cp) {
    constexpr int ICB = kGnStage / (25 * CO), WS = CO + 4, NT = CO / 32;
    const int lane = threadIdx.x & 63;
    const float *wl = ws + (lane >> 5) * 25 * WS + (lane & 31);
#pragma unroll 1
    for (int pr = 0; pr < ICB / 2; ++pr) {
        const float *ip = in + 2 * pr * cp, *wp = wl + 2 * pr * 25 * WS;
#pragma unroll 1
        for (int ky = 0; ky < 5; ++ky)
#pragma unroll
            for (int kx = 0; kx < 5; ++kx) {
                float a[MT], b[NT];
#pragma unroll
                for (int n = 0; n < NT; ++n) b[n] = wp[(ky * 5 + kx) * WS + 32 * n];
#pragma unroll
                for (int j = 0; j < MT; ++j) a[j] = ip[ab[j] + ky * pitch + kx];
#pragma unroll
                for (int j = 0; j < MT; ++j)
#pragma unroll
                    for (int n = 0; n < NT; ++n)
                        acc[j][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b[n], acc[j][n], 0, 0, 0);
            }
    }
}

// the stage for a wave's own tile count (wave-uniform; the barriers stay outside)
template <int CO, int MT, int MTMAX>
__device__ __forceinline__ void gn_mma_pick(int my, floatx16 (&acc)[MTMAX][CO / 32], const float *in,
                                            const int (&ab)[MTMAX], const float *ws, int pitch, int cp) {
    if (my == MT) gn_mma_stage<CO, MT, MTMAX>(acc, in, ab, ws, pitch, cp);
    else if constexpr (MT < MTMAX) gn_mma_pick<CO, MT + 1, MTMAX>(my, acc, in, ab, ws, pitch, cp);
}

// 5 x 5 convolution, CI -> CO channels, zero padding 2, on the matrix cores: in = TS * CI channels
// of h x w in the shared-halo layout, out [TS, CO, h, w] compact (bias added), which may lie over
// `in`.  wg: the weights [CO, CI, 5, 5] of the job's row, bg the bias.
// TR: the data gradient of such a convolution instead (gn_conv's TR): wg is the forward weight
// [CI, CO, 5, 5], the stage holds tap 24 - k of (k-channel c, output o) at k row (c, k) -- the taps
// are flipped when the stage is written, A is read as in the forward -- and there is no bias.
template <int CO, int CI, bool TR, int TS, int MTMAX>
__device__ __forceinline__ void gn_conv_mfma(const float *in, float *out, int h, int w,
                                             const float *__restrict__ wg, const float *__restrict__ bg,
                                             float *ws) {
    constexpr int ICB = kGnStage / (25 * CO), KR = ICB * 25, WS = CO + 4, NST = CI / ICB;
    constexpr int NPRE = kGnStage / 256, NT = CO / 32;
    static_assert(KR * WS <= kGnWFloats && NPRE * 256 == kGnStage && ICB % 2 == 0, "stage size");
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, half = lane >> 5, col = lane & 31;
    const int pitch = w + 2, cp = gn_halo_cp(h, w), hw = h * w, m_all = TS * hw;
    const int n_mt = (m_all + 31) / 32;
    const int my = __builtin_amdgcn_readfirstlane(wave < n_mt ? (n_mt - wave + 3) / 4 : 0);
    int ab[MTMAX];                               // this lane's A row in M-tile j: (sample, channel half, y, x)
    floatx16 acc[MTMAX][NT];
#pragma unroll
    for (int j = 0; j < MTMAX; ++j) {
        const int m = (wave + 4 * j) * 32 + col, mm = m < m_all ? m : 0;      // padding rows read row 0
        const int s = mm / hw, pos = mm % hw;
        ab[j] = (s * CI + half) * cp + (pos / w) * pitch + pos % w;
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[j][n][r] = 0.f;
    }
    float pre[NPRE];
    auto fetch = [&](int st) {                   // gn_conv's: element e is channel e / KR, k row e % KR
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
        __syncthreads();                         // the previous stage has been read
#pragma unroll
        for (int q = 0; q < NPRE; ++q) {
            const int e = q * 256 + tid;
            ws[(e % KR) * WS + e / KR] = pre[q];
        }
        __syncthreads();
        if (st + 1 < NST) fetch(st + 1);
        gn_mma_pick<CO, 1, MTMAX>(my, acc, in + st * ICB * cp, ab, ws, pitch, cp);
    }
    __syncthreads();                             // every wave has read `in`: out may lie over it
#pragma unroll
    for (int j = 0; j < MTMAX; ++j) {
        if (j >= my) continue;                   // wave-uniform
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const int oc = n * 32 + col;
            float b = 0.f;
            if constexpr (!TR) b = bg[oc];
#pragma unroll
            for (int r = 0; r < 16; ++r) {       // D row of register r: k_mix_dense's mapping
                const int m = (wave + 4 * j) * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (m < m_all) {
                    const int s = (m >= hw) + (m >= 2 * hw) + (m >= 3 * hw);      // TS <= 4
                    out[(s * CO + oc) * hw + m - s * hw] = TR ? acc[j][n][r] : acc[j][n][r] + b;
                }
            }
        }
    }
    __syncthreads();
}

// the kernel's own barriers: inlined here first, as its other functions' are (the kernel's target
// attribute keeps a plain __syncthreads() in its body a call)
__device__ __forceinline__ void gn_sync() { __syncthreads(); }

// Compiled without the packed fp32 VALU forms (v_pk_fma_f32 and kin): the kernel's scalar fp32 work
// is conv1's, whose fmas give the same bits either way.
template <int TS>
__global__ __launch_bounds__(256) __attribute__((target("no-packed-fp32-ops"))) void k_gnl_eval_mfma(const float *__restrict__ theta, int64_t ld_t,
                                                       const float *__restrict__ data,
                                                       const int32_t *__restrict__ labels,
                                                       const int32_t *__restrict__ rows,
                                                       const int32_t *__restrict__ seg_start,
                                                       const int32_t *__restrict__ seg_len, int64_t n_jobs,
                                                       int max_len, int n_tiles, const GnShape g,
                                                       double *__restrict__ part_loss,
                                                       int32_t *__restrict__ part_cnt,
                                                       int32_t *__restrict__ pred, int64_t ld_pred,
                                                       float *__restrict__ logits, int64_t ld_logits) {
    static_assert(TS == 2 || TS == 4, "gn_conv_mfma's write-back and the statistics' 16 floats hold 4 samples");
    extern __shared__ __attribute__((aligned(16))) float gn_smem[];
    float *ws = gn_smem, *stat = gn_smem + kGnWFloats, *buf = stat + 16 + 2 * TS * 64;
    const int tid = threadIdx.x;
    const int hw1 = g.h1 * g.w1, hw2 = g.h2 * g.w2;
    float *x3 = buf + TS * 32 * hw1;             // conv3's halo'd input, behind conv2's compact output
    float *feat = buf + TS * 64 * hw2;           // the features, behind conv3's compact output
    const int64_t n_work = n_jobs * n_tiles, sample = (int64_t)g.Cin * g.H * g.W;
    for (int64_t wk = blockIdx.x; wk < n_work; wk += gridDim.x) {       // wk = job * n_tiles + tile
        const int64_t job = wk / n_tiles;
        const int t = (int)(wk % n_tiles);
        const int left = ev_len(seg_len, job, max_len) - t * TS;
        if (left <= 0) continue;                                      // block-uniform
        const int ns = left < TS ? left : TS;
        const int64_t s0 = (int64_t)seg_start[job] + (int64_t)t * TS;
        const float *th = theta + (int64_t)rows[job] * ld_t;

        const float *x0 = data + s0 * sample;
        gn_conv1_pool<false, TS>([&](int s) { return x0 + (int64_t)(s < ns ? s : 0) * sample; }, g, th, buf, ws);
        gn_stats<32, TS>(buf, hw1, th + g.g1w, th + g.g1b, stat);
        gn_halo_expand<TS * 32>(buf, g.h1, g.w1, stat);
        gn_conv_mfma<32, 32, false, TS, kGnMfmaMT2>(buf, buf, g.h1, g.w1, th + g.c2w, th + g.c2b, ws);
        gn_stats<32, TS>(buf, hw1, th + g.g2w, th + g.g2b, stat);
        gn_halo_zero(x3, TS * 32, g.h2, g.w2);
        gn_norm_pool<32, TS, true>(buf, x3, g.h1, g.w1, g.h2, g.w2, stat);
        gn_conv_mfma<64, 32, false, TS, kGnMfmaMT3>(x3, buf, g.h2, g.w2, th + g.c3w, th + g.c3b, ws);
        gn_stats<64, TS>(buf, hw2, th + g.g3w, th + g.g3b, stat);
        gn_norm_pool<64, TS>(buf, feat, g.h2, g.w2, g.h3, g.w3, stat);

        gn_linear<TS>(feat, g, th, ws);
        if (logits)
            for (int e = tid; e < ns * g.C; e += 256)
                logits[(job * ld_logits + (int64_t)t * TS) * g.C + e] = ws[e];
        if (tid < ns) {
            const int y = labels[s0 + tid];
            EvState q;
            ev_scan(ws + tid * g.C, g.C, 0, y, true, q);
            stat[8 + tid] = (q.best + logf(q.sum)) - q.zy;
            stat[8 + TS + tid] = q.idx == y ? 1.f : 0.f;
            if (pred) pred[job * ld_pred + (int64_t)t * TS + tid] = q.idx;
        }
        gn_sync();
        if (tid == 0) {                                               // in sample order
            double a = 0.0;
            int c = 0;
            for (int s = 0; s < ns; ++s) {
                a += (double)stat[8 + s];
                c += stat[8 + TS + s] != 0.f;
            }
            part_loss[wk] = a;
            part_cnt[wk] = c;
        }
        gn_sync();                                              // ws, stat and the buffer are free
    }
}
