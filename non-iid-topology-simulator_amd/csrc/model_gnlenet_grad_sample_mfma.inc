// GN-LeNet training with the sample pass's conv2 / conv3 on the matrix cores
// (k_gnl_grad_sample_mfma, niidmix_gnlenet_nll_grad_rows_mfma_sample_f32).  Included by niidmix.hip
// after model_gnlenet_grad_mfma.inc; it uses gn_conv_mfma, gn_halo_expand and gn_halo_zero of
// model_gnlenet_mfma.inc and the VALU functions of model_gnlenet.inc.
// ----------------------------------------------------------------------------------------------
// k_gnl_grad_sample_mfma<true> (niidmix_gnlenet_nll_grad_rows_mfma_fwd1_f32) runs conv1 there as well,
// through gn_conv1_pool_mfma of model_gnlenet_conv1_mfma.inc; what follows describes both.
// Job model, scratch slot (GnGradLay) and outputs are k_gnl_grad_sample's: one work item per (row
// entry, tile of kGnTS = 2 samples) on a persistent grid, and every array a later kernel reads
// (p1, x2, y2, dy2, dx2, x3, y3, dy3, feat, dz, nll, st1..3, gp1..3, amax) lands in the slot in the
// same compact layout, so k_gnl_grad_wmfma, k_gnl_grad_conv<false> and k_gnl_grad_fc follow
// unmodified.  dx3 and dfeat live in LDS only; their places in the slot stay unwritten.
// Four implicit GEMMs per tile on v_mfma_f32_32x32x2_f32 (gn_conv_mfma: M = the tile's output
// positions over both samples in M-tiles of 32, wave w owns M-tiles w, w + 4, ...):
//   GEMM                         M          N    K         weight stages of 8 k-channels x 25 x 32
//   conv2 forward                2 h1 w1    32   32 x 25   4
//   conv3 forward                2 h2 w2    64   32 x 25   8 (of 4 k-channels x 25 x 64)
//   conv3 data gradient -> dX3   2 h2 w2    32   64 x 25   8
//   conv2 data gradient -> dX2   2 h1 w1    32   32 x 25   4
// The data gradients FLIP THE TAPS WHEN THE STAGE IS WRITTEN (gn_conv's TR indexing: k row (c, k)
// of the stage holds w[c][o][24 - k]); A is read at ky * pitch + kx in all four, so the MFMA loop
// (gn_mma_stage) is one and the same.  The gradient maps enter the shared-halo layout unchanged
// (gn_halo_expand<NCH, false>), dY3 as 2 x 64 channels.
// LDS: the weight stage (kGnWFloats), the statistics (kGnStat) and ONE activation buffer `buf`,
// which carries each GEMM's halo'd operand and receives its compact result.  With a1 = 2 * 32 h1 w1,
// a2 = 2 * 32 h2 w2, cpN = (hN + 2)(wN + 2), F the features per sample, its map per step is
//   conv1 / GroupNorm 1   [0, a1) p1, then x2 in place (both copied to the slot)
//   conv2                 [0, 64 cp1 + tail) x2 halo'd, expanded in place; y2 compact over it
//   pool 2                [0, a1) y2 | [a1, a1 + 64 cp2 + tail) x3 halo'd (copied compact to the slot)
//   conv3 .. classifier   [0, 2 a2) y3 | feat [2 F] | dfeat [2 F]
//   pool / norm 3 back    ... | [2 a2 + 4 F, + 2 a2) dy3 compact, then + 128 cp2 + tail halo'd in place
//   conv3 data gradient   [a1, a1 + a2) dx3 compact (over the halo'd dY3 where they meet)
//   pool / norm 2 back    [0, a1) dy2 compact (y2, x3 and st2 re-read from the slot) | dx3
//   conv2 data gradient   [0, 64 cp1 + tail) dY2 halo'd in place; dx2 compact over it
//   ReLU, norm 1 back     [0, a1) dx2 in place (x2, p1, st1 from the slot), copied to the slot
// gn_gsm_act_floats is the largest of these; at every shape gn_mfma_ts takes at two samples the
// backward's steps fit where the forward's do (20 x 20 pooled maps: 29976 against 33368 floats),
// and the launcher checks it.  The statistics of a stage are read from LDS by its backward (stage 3's
// are still there; 2's and 1's come back from the slot), gn_norm_bwd's 8 floats of `red` are
// stat[8..16), which this kernel does not use otherwise.
// Contract: k_gnl_grad_sample's, with conv2's, conv3's and the two data gradients' outputs each one
// K-order chain (stage, channel pair, ky, kx; the pair's two channels in order) whatever the output's
// position in M; no atomics; theta is not written.  A halo position contributes 0 * w: a
// non-finite weight reaches the border outputs too, within its own row.
inline int64_t gn_gsm_act_floats(const GnShape &g) {
    const int64_t a1 = kGnTS * 32 * g.h1 * g.w1, a2 = kGnTS * 32 * g.h2 * g.w2;
    const int64_t cp1 = gn_halo_cp(g.h1, g.w1), cp2 = gn_halo_cp(g.h2, g.w2);
    const int64_t c2 = kGnTS * 32 * cp1 + gn_halo_tail(g.w1);                  // conv2 and its data gradient
    const int64_t c3 = a1 + kGnTS * 32 * cp2 + gn_halo_tail(g.w2);             // y2 | x3 halo'd
    const int64_t b3 = 2 * a2 + 2 * kGnTS * g.F + kGnTS * 64 * cp2 + gn_halo_tail(g.w2);   // y3 | feat | dfeat | dY3
    const int64_t m = c2 > c3 ? c2 : c3;                                       // a1 + a2 (dy2 | dx3) < c3
    return m > b3 ? m : b3;
}
inline int64_t gn_gsm_lds_bytes(const GnShape &g) { return (kGnWFloats + kGnStat + gn_gsm_act_floats(g)) * 4; }
// the shapes the kernel takes: gn_mfma_ts' at two samples (the M-tiles a wave holds, the forward's
// buffer), and the backward's buffer within the same bound
inline bool gn_gsm_takes(const GnShape &g) { return gn_mfma_ts(g) >= 2 && gn_gsm_lds_bytes(g) <= kGnLdsMax; }

// n floats of LDS to the slot; no barrier
__device__ __forceinline__ void gn_gsm_store(float *dst, const float *src, int n) {
    for (int e = threadIdx.x; e < n; e += 256) dst[e] = src[e];
}

// C1M: conv1 + pool as gn_conv1_pool_mfma (model_gnlenet_conv1_mfma.inc), its stage behind p1 in
// `buf` (and in the unused part of `ws`), in a dynamic LDS of gn_c1_geom's size where that is more;
// every later step is the same.  <false> is the kernel as it was.
template <bool C1M>
__global__ __launch_bounds__(256) void k_gnl_grad_sample_mfma(const float *__restrict__ theta, int64_t ld_t,
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
    float *ws = gn_smem, *stat = gn_smem + kGnWFloats, *buf = stat + kGnStat, *red = stat + 8;
    const int tid = threadIdx.x;
    const int hw1 = g.h1 * g.w1, hw2 = g.h2 * g.w2, a1 = kGnTS * 32 * hw1, a2 = kGnTS * 32 * hw2;
    const int nf = kGnTS * g.F;
    float *x3 = buf + a1, *dx3 = buf + a1;       // conv3's halo'd input behind y2; dx3 behind dy2
    float *feat = buf + 2 * a2, *dfeat = feat + nf, *dy3 = dfeat + nf;      // behind y3
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

        // forward: every map passes through LDS and is kept in the slot
        if constexpr (C1M)
            gn_conv1_pool_mfma<true>([&](int s) { return data + (int64_t)bi[s < ns ? s : 0] * sample; }, g, th,
                                     buf, ws, buf + a1, gn_c1_geom(g.Cin, g.H, g.W, kGnTS, kGnWFloats + kGnStat),
                                     reinterpret_cast<unsigned char *>(T + L.amax));
        else
            gn_conv1_pool<true>([&](int s) { return data + (int64_t)bi[s < ns ? s : 0] * sample; }, g, th,
                                buf, ws, reinterpret_cast<unsigned char *>(T + L.amax));
        gn_stats<32>(buf, hw1, th + g.g1w, th + g.g1b, stat);
        gn_gsm_store(T + L.st1, stat, kGnStat);
        for (int e = tid; e < a1; e += 256) {
            const float p = buf[e];
            const float v = gn_relu(__builtin_fmaf(p, stat[16 + 2 * (e / hw1)], stat[16 + 2 * (e / hw1) + 1]));
            T[L.p1 + e] = p;
            T[L.x2 + e] = v;
            buf[e] = v;
        }
        __syncthreads();
        gn_halo_expand<kGnTS * 32, false>(buf, g.h1, g.w1, nullptr);
        gn_conv_mfma<32, 32, false, kGnTS, kGnMfmaMT2>(buf, buf, g.h1, g.w1, th + g.c2w, th + g.c2b, ws);
        gn_gsm_store(T + L.y2, buf, a1);
        gn_stats<32>(buf, hw1, th + g.g2w, th + g.g2b, stat);
        gn_gsm_store(T + L.st2, stat, kGnStat);
        gn_halo_zero(x3, kGnTS * 32, g.h2, g.w2);
        gn_norm_pool<32, kGnTS, true>(buf, x3, g.h1, g.w1, g.h2, g.w2, stat);
        for (int e = tid; e < a2; e += 256) {                         // x3, compact, to the slot
            const int sc = e / hw2, pos = e % hw2;
            T[L.x3 + e] = x3[sc * gn_halo_cp(g.h2, g.w2) + (pos / g.w2 + 2) * (g.w2 + 2) + pos % g.w2 + 2];
        }
        gn_conv_mfma<64, 32, false, kGnTS, kGnMfmaMT3>(x3, buf, g.h2, g.w2, th + g.c3w, th + g.c3b, ws);
        gn_gsm_store(T + L.y3, buf, 2 * a2);
        gn_stats<64>(buf, hw2, th + g.g3w, th + g.g3b, stat);
        gn_gsm_store(T + L.st3, stat, kGnStat);
        gn_norm_pool<64>(buf, feat, g.h2, g.w2, g.h3, g.w3, stat);
        gn_gsm_store(T + L.feat, feat, nf);
        gn_linear(feat, g, th, ws);

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
        for (int e = tid; e < nf; e += 256) {                         // the feature gradient
            const int s = e / g.F, f = e % g.F;
            const float *wc = th + g.fw + f;
            float acc = 0.f;
            for (int c = 0; c < g.C; ++c) acc = __builtin_fmaf(ws[s * g.C + c], wc[(int64_t)c * g.F], acc);
            dfeat[e] = acc;
        }
        __syncthreads();

        // backward: stage 3 on what LDS still holds (y3, feat, its statistics)
        gn_pool_bwd<64>(buf, feat, dfeat, dy3, g.h2, g.w2, g.h3, g.w3, stat);
        gn_norm_bwd<64>(buf, dy3, hw2, th + g.g3w, stat, T + L.gp3, red);
        gn_gsm_store(T + L.dy3, dy3, 2 * a2);
        gn_halo_expand<kGnTS * 64, false>(dy3, g.h2, g.w2, nullptr);
        gn_conv_mfma<32, 64, true, kGnTS, kGnMfmaMT3>(dy3, dx3, g.h2, g.w2, th + g.c3w, nullptr, ws);
        // stage 2: y2, x3 and the statistics from the slot, dy2 and dx3 in LDS
        gn_gsm_store(stat, T + L.st2, kGnStat);
        __syncthreads();
        gn_pool_bwd<32>(T + L.y2, T + L.x3, dx3, buf, g.h1, g.w1, g.h2, g.w2, stat);
        gn_norm_bwd<32>(T + L.y2, buf, hw1, th + g.g2w, stat, T + L.gp2, red);
        gn_gsm_store(T + L.dy2, buf, a1);
        gn_halo_expand<kGnTS * 32, false>(buf, g.h1, g.w1, nullptr);
        gn_conv_mfma<32, 32, true, kGnTS, kGnMfmaMT2>(buf, buf, g.h1, g.w1, th + g.c2w, nullptr, ws);
        // stage 1: the ReLU's mask from x2, GroupNorm on p1
        for (int e = tid; e < a1; e += 256)
            if (T[L.x2 + e] <= 0.f) buf[e] = 0.f;                     // ReLU; a NaN passes
        gn_gsm_store(stat, T + L.st1, kGnStat);
        __syncthreads();
        gn_norm_bwd<32>(T + L.p1, buf, hw1, th + g.g1w, stat, T + L.gp1, red);
        gn_gsm_store(T + L.dx2, buf, a1);
        __syncthreads();                                              // ws, stat and the buffer are free
    }
}
