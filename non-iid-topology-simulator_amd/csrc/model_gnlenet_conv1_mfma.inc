// GN-LeNet's conv1 + max-pool on the matrix cores (gn_conv1_pool_mfma; the sample pass
// k_gnl_grad_sample_mfma<true>, niidmix_gnlenet_nll_grad_rows_mfma_fwd1_f32).  Included by
// niidmix.hip after model_gnlenet_mfma.inc, whose halo helpers it uses.
// ----------------------------------------------------------------------------------------------
// gn_conv1_pool (model_gnlenet.inc) gives a lane the nine conv outputs under its pool window, so the
// stride-2 windows compute every conv output about twice, on the VALU.  Here every conv output is
// computed once per band, as a BANDED implicit GEMM on v_mfma_f32_32x32x2_f32, and pooled from LDS:
//   M   the full-resolution output positions (row, column) of one band of one sample, flattened
//       over the we = 2 w1 + 1 columns that lie in a window (an even W's last column is in none),
//       in M-tiles of 32 that may straddle rows; wave w takes M-tiles w, w + 4, ... one at a time,
//       16 accumulators each.  Padding rows of the last M-tile read position 0 and are not written
//   N   the 32 output channels
//   K   25 Cin <= 100 in the order (ci, ky, kx) ascending, gn_conv1_pool's chain; the two lane
//       halves of an MFMA take k = 2 t and 2 t + 1.  An odd K (Cin 1, 3) has one pad k: its B
//       value is zero and its A value is a zero that is not read from the data
//   B   read once per work item from gn_conv1_pool's [k][32 + 4] weights in `ws` into registers
//       (<= 50 per lane), with the lane's <= 50 A offsets ci chan + ky pitch + kx beside them
//   A   one ds_read_b32 per lane and K-step at base + offset, no bounds test: the INPUT BAND holds,
//       per input channel, 2 pb + 5 rows of pitch W + 2 in the shared-halo convention (pixel (Y, X)
//       of band row r at r pitch + X + 2; columns 0, 1 zero, a row's right halo the next row's left
//       one; rows outside the map zero; gn_halo_tail zeros behind the last channel)
//   D   the CONV BAND [32][chs], chs = ((2 pb + 1) we) | 1 odd, written from the accumulators in
//       gn_conv_mfma's D mapping m = (r & 3) + 8 (r >> 2) + 4 half
// A STAGE is (sample, band of pb pooled rows): conv rows 2 r0 .. 2 r0 + 2 pb from input rows
// 2 r0 - 2 .. 2 r0 + 2 pb + 2.  The one conv row two consecutive bands share is RECOMPUTED (a band
// then depends on nothing but its own input rows; a carried row would cost a copy through LDS of the
// same size).  Per stage: fill the input band | barrier | MFMAs, conv band | barrier | pool.  The
// next fill writes the input band only, which the MFMAs have left, so it runs beside the pool.
// Pool: eight lanes per channel (its bias in a register) stride the band's (pooled row, pooled
// column) positions; a lane reads its nine conv outputs in window order, keeps the first maximum
// under gn_max's rule (a NaN wins and stays), adds the bias after the maximum and writes `out` and,
// when AM, the argmax byte.  The stride-2 reads are 2-way bank conflicts and are accepted.
// Contract: gn_conv1_pool's.  Every conv output is one K-order chain from 0 whatever its place in
// M and its band; a halo position contributes 0 * w, so a non-finite weight reaches border outputs
// too (as it does through gn_conv1_pool's zero patch values).
struct GnC1Geom {
    int pitch, we, pb;               // input row pitch, conv columns kept, pooled rows per band (0: none fits)
    int chan, chs;                   // channel strides of the input band and of the conv band
    bool in_ws;                      // the input band lives in the unused part of `ws`, else behind the conv band
    int lds_floats;                  // the end of the stage in the kernel's dynamic LDS
};

// The stage next to out [ts, 32, h1, w1] at float act_off of the kernel's LDS: the conv band
// follows `out`; the input band goes behind the weights in `ws` when it fits there, else behind the
// conv band.  pb is the largest value whose stage ends within kGnLdsMax less 64 B.
__host__ __device__ __forceinline__ GnC1Geom gn_c1_geom(int cin, int h, int w, int ts, int act_off) {
    GnC1Geom q;
    const int h1 = gn_down(h), w1 = gn_down(w), kp = (cin * 25 + 1) & ~1;
    q.pitch = w + 2;
    q.we = 2 * w1 + 1;
    const int cv = act_off + ts * 32 * h1 * w1;
    for (q.pb = h1; q.pb >= 1; --q.pb) {
        q.chan = (2 * q.pb + 5) * q.pitch;
        q.chs = ((2 * q.pb + 1) * q.we) | 1;
        const int inf = cin * q.chan + gn_halo_tail(w);
        q.in_ws = inf <= kGnWFloats - kp * (32 + 4);
        q.lds_floats = cv + 32 * q.chs + (q.in_ws ? 0 : inf);
        if (q.lds_floats <= (int)(kGnLdsMax / 4) - 16) break;       // the kernel's static LDS (16 B) stays free
    }
    return q;
}

template <int CIN, bool AM, int TS, class XOf>
__device__ __forceinline__ void gn_c1_bands(XOf xof, const GnShape &g, const float *__restrict__ th,
                                            float *out, const float *ws, float *cv, float *in,
                                            const GnC1Geom &q, unsigned char *amax) {
    constexpr int WS = 32 + 4, NK = CIN * 25, KS = (NK + 1) / 2, FILL = 4;
    const int tid = threadIdx.x, wave = wave_id(), lane = tid & 63, half = lane >> 5, col = lane & 31;
    const int H = g.H, W = g.W, h1 = g.h1, w1 = g.w1, hw1 = h1 * w1;
    const int oc = tid >> 3;                     // the pool's channel of this lane
    const float bias = th[g.c1b + oc];
    float b[KS];
    int ko[KS];
#pragma unroll
    for (int t = 0; t < KS; ++t) {
        const int k = 2 * t + half, kk = k < NK ? k : 0, tap = kk % 25;
        ko[t] = (kk / 25) * q.chan + (tap / 5) * q.pitch + tap % 5;
        b[t] = k < NK ? ws[k * WS + col] : 0.f;
    }
    // the zeros no fill writes: columns 0, 1 of every row, the tail
    for (int it = tid; it < CIN * (2 * q.pb + 5); it += 256) in[it * q.pitch] = in[it * q.pitch + 1] = 0.f;
    for (int e = tid; e < gn_halo_tail(W); e += 256) in[CIN * q.chan + e] = 0.f;
#pragma unroll 1
    for (int s = 0; s < TS; ++s) {
        const float *xs = xof(s);
#pragma unroll 1
        for (int r0 = 0; r0 < h1; r0 += q.pb) {
            const int pbn = h1 - r0 < q.pb ? h1 - r0 : q.pb, cr = 2 * pbn + 1, irn = cr + 4;
            const int m_all = cr * q.we, n_mt = (m_all + 31) / 32, nfill = CIN * irn * W;
            // the input band: element e is (channel, band row, pixel), FILL loads in flight
#pragma unroll 1
            for (int e0 = tid; e0 < nfill; e0 += 256 * FILL) {
                float v[FILL];
                int d[FILL];
#pragma unroll
                for (int u = 0; u < FILL; ++u) {
                    const int e = e0 + 256 * u, ee = e < nfill ? e : 0;
                    const int it = ee / W, x = ee % W, ci = it / irn, rr = it % irn, y = 2 * r0 - 2 + rr;
                    const bool ok = e < nfill && (unsigned)y < (unsigned)H;
                    v[u] = ok ? xs[((int64_t)ci * H + (ok ? y : 0)) * W + x] : 0.f;
                    d[u] = e < nfill ? ci * q.chan + rr * q.pitch + x + 2 : -1;
                }
#pragma unroll
                for (int u = 0; u < FILL; ++u)
                    if (d[u] >= 0) in[d[u]] = v[u];
            }
            __syncthreads();                     // the band is filled; the last pool has read the conv band
#pragma unroll 1
            for (int mt = wave; mt < n_mt; mt += 4) {
                const int m = mt * 32 + col, mm = m < m_all ? m : 0;
                const float *ap = in + (mm / q.we) * q.pitch + mm % q.we;
                floatx16 acc;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
                for (int t = 0; t < KS; ++t) {
                    float a = ap[ko[t]];
                    if ((NK & 1) && t == KS - 1) a = half ? 0.f : a;         // the pad k
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b[t], acc, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int mo = mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                    if (mo < m_all) cv[col * q.chs + mo] = acc[r];
                }
            }
            __syncthreads();
            for (int e = tid & 7; e < pbn * w1; e += 8) {            // 8 lanes per channel: its bias is a register
                const int pj = e % w1, pi = e / w1;
                const float *p = cv + oc * q.chs + 2 * pi * q.we + 2 * pj;
                float m = p[0];
                int am = 0;
#pragma unroll
                for (int a = 1; a < 9; ++a) {
                    const float v = p[(a / 3) * q.we + a % 3];
                    if (AM && (v > m || v != v)) am = a;
                    m = gn_max(m, v);
                }
                const int o = (s * 32 + oc) * hw1 + (r0 + pi) * w1 + pj;
                out[o] = m + bias;
                if constexpr (AM) amax[o] = (unsigned char)am;
            }
        }
    }
    __syncthreads();
}

// gn_conv1_pool's arguments and results; stage = the conv band's place in LDS (behind `out`), q =
// gn_c1_geom's answer for the shape, the tile size and out's place.
template <bool AM = false, int TS = kGnTS, class XOf>
__device__ __forceinline__ void gn_conv1_pool_mfma(XOf xof, const GnShape &g, const float *__restrict__ th,
                                                   float *out, float *ws, float *stage, const GnC1Geom &q,
                                                   unsigned char *amax = nullptr) {
    constexpr int WS = 32 + 4;
    const int nk = g.Cin * 25;
    for (int e = threadIdx.x; e < 32 * nk; e += 256) ws[(e % nk) * WS + e / nk] = th[g.c1w + e];
    __syncthreads();
    float *in = q.in_ws ? ws + ((nk + 1) & ~1) * WS : stage + 32 * q.chs;
    switch (g.Cin) {                             // block-uniform: K's length is a compile-time constant
    case 1: gn_c1_bands<1, AM, TS>(xof, g, th, out, ws, stage, in, q, amax); break;
    case 2: gn_c1_bands<2, AM, TS>(xof, g, th, out, ws, stage, in, q, amax); break;
    case 3: gn_c1_bands<3, AM, TS>(xof, g, th, out, ws, stage, in, q, amax); break;
    default: gn_c1_bands<4, AM, TS>(xof, g, th, out, ws, stage, in, q, amax); break;
    }
}
