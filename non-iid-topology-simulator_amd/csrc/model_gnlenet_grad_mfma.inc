// GN-LeNet training with the conv2 / conv3 weight gradients on the matrix cores (k_gnl_grad_wmfma,
// niidmix_gnlenet_nll_grad_rows_mfma_f32).  Included by niidmix.hip after model_gnlenet_mfma.inc;
// it reads the scratch slots that k_gnl_grad_sample (model_gnlenet.inc) left.
// ----------------------------------------------------------------------------------------------
// Per row and layer the weight gradient is one GEMM on v_mfma_f32_32x32x2_f32,
//   dW[co, (ci, ky, kx)] = sum_s sum_(y, x) dY[s, co, y, x] Xpad[s, ci, y + ky - 2, x + kx - 2]:
//   M   32 output channels: a UNIT is conv2, conv3 channels 0..31 or conv3 channels 32..63
//   N   800 = 25 taps x 32 input channels, cut in 25 N-tiles of one tap each; wave w of the
//       unit's workgroup owns taps w, w + 4, ... (7 / 6 / 6 / 6) and keeps their accumulators in
//       registers through the whole K loop
//   K   (sample in batch order, band of map rows, position in the band's PITCHED map): q walks a
//       band's rows of pitch w + 2 linearly, two consecutive q per MFMA (the two lane halves)
// One workgroup per (row, unit); the conv2 units, about 4 x as long, come first in the grid.
// A STAGE is what the workgroup holds in LDS at a time: ns samples of one band of bh map rows
// (gn_wm_geom: the whole map and as many samples as fit where a sample fits, else one sample and
// the fewest bands of equal height that fit).  Per sample and channel
//   X    bh + 4 rows of pitch w + 2: the band's rows and two above and below (zero outside the
//        map), pixel (r, x) at r * pitch + x + 2.  Columns 0, 1 of a row are zero and are the
//        right halo of the row before; a band's rows above and below are data in the middle of a
//        map, so -- unlike k_gnl_eval_mfma's layout -- a channel's bottom rows are its own
//   dY   bh rows of the same pitch, pixel (r, x) at q = r * pitch + x, columns w, w + 1 zero
// and then A[m][q] = dY[m * chanA + q], B[n][q] = X[n * chanX + q + ky * pitch + kx]: one
// ds_read_b32 per lane and K-step for A, one per MFMA for B at a constant tap offset, no bounds
// test.  The channel strides chanA, chanX are odd (the 32 lanes of a read hit 32 banks); K per
// (sample, band) is bh * pitch - 2, padded to even with a position whose dY is zero.  The zero
// positions are written once per workgroup, a stage's fill writes pixels only (rows outside the
// map and samples outside the stage as zeros).  The stage is kGnWmFloats at most, so that two
// workgroups share a CU and one multiplies while the other fills.
// Every output is one K-ordered chain: samples in batch order, bands top down, q ascending.  A
// halo position contributes 0 * x: a non-finite activation reaches every tap of its channel, the
// border taps that k_gnl_grad_conv's loop bounds would have kept it from included.
// Write-out: the unit's [32, 800] block of the row's gradient is contiguous; it goes through the
// then-free LDS in two halves of 16 output channels, so the global stores are coalesced.
constexpr int kGnWmFloats = 19968;               // 78 KiB of LDS per workgroup
constexpr int kGnWmTiles = 7;                    // N-tiles (taps) a wave owns at most
constexpr int kGnWmFill = 4;                     // global loads a thread of the fill keeps in flight

struct GnWmGeom {
    int pitch, bh, nb, ns;                       // row pitch, rows per band, bands, samples per stage
    int chanX, chanA, ksteps;                    // channel strides, MFMAs per (sample, band, tile)
};

__host__ __device__ __forceinline__ int gn_wm_sample_floats(int bh, int pitch) {
    return 32 * ((((bh + 4) * pitch) | 1) + ((bh * pitch) | 1));
}

__host__ __device__ __forceinline__ GnWmGeom gn_wm_geom(int h, int w) {
    GnWmGeom q;
    q.pitch = w + 2;
    int bh = h;
    while (gn_wm_sample_floats(bh, q.pitch) + 8 > kGnWmFloats) --bh;     // bh >= 1 up to 31 x 31 maps
    q.nb = (h + bh - 1) / bh;
    q.bh = (h + q.nb - 1) / q.nb;
    q.ns = q.nb == 1 ? (kGnWmFloats - 8) / gn_wm_sample_floats(h, q.pitch) : 1;
    q.chanX = ((q.bh + 4) * q.pitch) | 1;
    q.chanA = (q.bh * q.pitch) | 1;
    q.ksteps = (q.bh * q.pitch - 1) / 2;         // K = bh * pitch - 2, rounded up to even
    return q;
}

// floats of a unit's LDS: the stage (4 floats follow the last channel of X and of dY: a B read
// ends 3 past it, gn_wm_steps' read ahead 4 past X and 1 past dY) or one half of the write-out
__host__ __device__ __forceinline__ int gn_wm_lds_floats(const GnWmGeom &q) {
    const int st = q.ns * 32 * (q.chanX + q.chanA) + 8;
    return st > 16 * 800 ? st : 16 * 800;
}

// the K-steps of one (sample, band): ap / bp are this lane's A and B addresses at q = 0 (its row,
// its lane half), toff the offsets of the wave's taps
__device__ __forceinline__ void gn_wm_steps(floatx16 (&acc)[kGnWmTiles], const float *ap, const float *bp,
                                            const int (&toff)[kGnWmTiles], int ksteps) {
    const float *bt[kGnWmTiles];
#pragma unroll
    for (int j = 0; j < kGnWmTiles; ++j) bt[j] = bp + toff[j];
    // the next step's operands are read before this step's MFMAs issue; the read past the last
    // step stays inside the workgroup's LDS (gn_wm_lds_floats) and is not used
    float a = ap[0], b[kGnWmTiles];
#pragma unroll
    for (int j = 0; j < kGnWmTiles; ++j) b[j] = bt[j][0];
#pragma unroll 1
    for (int k = 1; k <= ksteps; ++k) {
        const float an = ap[2 * k];
        float bn[kGnWmTiles];
#pragma unroll
        for (int j = 0; j < kGnWmTiles; ++j) bn[j] = bt[j][2 * k];
#pragma unroll
        for (int j = 0; j < kGnWmTiles; ++j)
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b[j], acc[j], 0, 0, 0);
        a = an;
#pragma unroll
        for (int j = 0; j < kGnWmTiles; ++j) b[j] = bn[j];
    }
}

// A stage's pixels of one operand: nr rows per channel, from map row ya on, of 32 channels (c0 on,
// of nc per sample) of the slot array at src0 in the row's first slot, for the samples s0 .. s0 + ns
// of the batch, to dst0 with channel stride chan; rows outside the map as zeros.  1 << lsh lanes
// along a map row (w <= 31), 256 >> lsh (sample, channel, row) items at a time, kGnWmFill of them in
// flight per thread.  No barrier.
__device__ __forceinline__ void gn_wm_fill(float *dst0, int chan, int pitch, int nr, int ya,
                                           const float *__restrict__ src0, int tile, int nc, int c0,
                                           int s0, int ns, int h, int w, int lsh) {
    const int tx = threadIdx.x & ((1 << lsh) - 1), ty = threadIdx.x >> lsh;
    const int n = ns * 32 * nr, hw = h * w;
#pragma unroll 1
    for (int it0 = ty; it0 < n; it0 += kGnWmFill << (8 - lsh)) {
        float v[kGnWmFill];
        int d[kGnWmFill];
#pragma unroll
        for (int u = 0; u < kGnWmFill; ++u) {
            const int it = it0 + (u << (8 - lsh));
            const int sc = it / nr, r = it % nr, sl = sc >> 5, c = sc & 31;
            const int y = ya + r, s = s0 + sl;
            const bool in = it < n && tx < w;
            // sample s lives in tile s / kGnTS of the row, at place s % kGnTS
            const float *src = src0 + (int64_t)(s / kGnTS) * tile + ((s % kGnTS) * nc + c0 + c) * hw + y * w + tx;
            v[u] = in && (unsigned)y < (unsigned)h ? *src : 0.f;
            d[u] = in ? (sl * 32 + c) * chan + r * pitch + tx : -1;
        }
#pragma unroll
        for (int u = 0; u < kGnWmFill; ++u)
            if (d[u] >= 0) dst0[d[u]] = v[u];
    }
}

#ifdef __HIP_DEVICE_COMPILE__                    // the host pass does not know the feature
#define NIIDMIX_GN_NO_PK __attribute__((target("no-packed-fp32-ops")))
#else
#define NIIDMIX_GN_NO_PK
#endif

// The batch cut over several workgroups per row (model_gnlenet_grad_split_mfma.inc has the rule and
// the reduction): chunk c of a row holds its samples [c ch, min(len, (c + 1) ch)), and a row of len
// samples has max(1, ceil(len / ch)) chunks, whatever the call's other rows are.  part holds, per
// (row, chunk of b_max's nchm), the row's three weight blocks in the order conv2, conv3, conv1.
struct GnSplit {
    int ch, nchm;                                // samples per chunk; chunks of a batch of b_max
    float *part;                                 // [n_rows, nchm, gn_split_floats(Cin)]
};
constexpr int kGnSplitC3 = 32 * 800, kGnSplitC1 = 3 * 32 * 800;     // conv3's, conv1's block in a partial

__host__ __device__ __forceinline__ int gn_split_floats(int cin) { return kGnSplitC1 + 32 * cin * 25; }

// A (row, chunk) workgroup's samples [s_lo, s_hi) of the row's len.  True where the workgroup has
// nothing to do (its chunk lies past the row's last); part is set where the row has more than one
// chunk and the block goes to its partial slot, else the block goes straight to grad.
__device__ __forceinline__ bool gn_split_range(const GnSplit &sp, int64_t i, int c, int len, int cin,
                                               int &s_lo, int &s_hi, float *&part) {
    const int nch = len > sp.ch ? (len + sp.ch - 1) / sp.ch : 1;
    if (c >= nch) return true;
    if (nch > 1) {
        s_lo = c * sp.ch;
        s_hi = s_lo + sp.ch < len ? s_lo + sp.ch : len;
        part = sp.part + (i * sp.nchm + c) * gn_split_floats(cin);
    }
    return false;
}

// Compiled without the packed fp32 VALU forms, as k_gnl_eval_mfma is: the kernel has no fp32 VALU
// arithmetic of its own.  k_gnl_grad_wmfma<> is a workgroup per (row, unit) that walks the whole
// batch; k_gnl_grad_wmfma<GnSplit> takes that one argument more and is a workgroup per (row, unit,
// chunk), the chunk fastest, over the chunk's samples (a stage starts at the chunk's first sample).
template <class... SP>
__global__ __launch_bounds__(256, 2) NIIDMIX_GN_NO_PK void k_gnl_grad_wmfma(
        const int32_t *__restrict__ batch_len, int b_max, const int32_t *__restrict__ rows, int n_rows,
        int n_tiles, const GnShape g, const GnGradLay L, const float *__restrict__ scratch,
        float *__restrict__ grad, int64_t ld_g, const SP... sp) {
    extern __shared__ __attribute__((aligned(16))) float gn_smem[];
    constexpr bool SPLIT = sizeof...(SP) > 0;
    const int tid = threadIdx.x, wave = wave_id(), lane = tid & 63, half = lane >> 5, col = lane & 31;
    unsigned unit = blockIdx.x;
    if constexpr (SPLIT) unit /= (unsigned)(sp, ...).nchm;
    // the unit: conv2 of row `unit`, or a half of conv3's output channels
    const bool c2 = (int)unit < n_rows;
    const int64_t i = c2 ? unit : (unit - n_rows) / 2;
    const int co0 = c2 ? 0 : (int)((unit - n_rows) % 2) * 32;
    const int CO = c2 ? 32 : 64, h = c2 ? g.h1 : g.h2, w = c2 ? g.w1 : g.w2;
    const int o_x = c2 ? L.x2 : L.x3, o_dy = c2 ? L.dy2 : L.dy3;
    const GnWmGeom q = gn_wm_geom(h, w);
    const int len = lin_len(batch_len, i, b_max);
    int s_lo = 0, s_hi = len;
    float *part = nullptr;
    if constexpr (SPLIT)                         // block-uniform, before the first barrier
        if (gn_split_range((sp, ...), i, (int)(blockIdx.x % (unsigned)(sp, ...).nchm), len, g.Cin, s_lo, s_hi, part))
            return;
    float *xs = gn_smem, *as = gn_smem + q.ns * 32 * q.chanX + 4;

    // taps wave, wave + 4, ... < 25: 7 for wave 0, 6 for the others, whose seventh tile repeats
    // tap 0 and is not written (wave 0's seven set the stage's time between the barriers anyway)
    const int my = wave == 0 ? 7 : 6;
    int toff[kGnWmTiles];
    floatx16 acc[kGnWmTiles];
#pragma unroll
    for (int j = 0; j < kGnWmTiles; ++j) {
        const int t = wave + 4 * j < 25 ? wave + 4 * j : 0;
        toff[j] = (t / 5) * q.pitch + t % 5;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    }
    // the zeros of the layout (and of everything else): once
    for (int e = tid; e < q.ns * 32 * (q.chanX + q.chanA) + 8; e += 256) gn_smem[e] = 0.f;

    const float *ap = as + col * q.chanA + half, *bp = xs + col * q.chanX + half;
    // the fill: lw lanes along a map row (w <= 31), 256 / lw (sample, channel, row) items at a time,
    // kGnWmFill of them in flight per thread
    const int lsh = w <= 8 ? 3 : w <= 16 ? 4 : 5;
    const float *T0 = scratch + i * n_tiles * L.tile;       // the row's first slot
#pragma unroll 1
    for (int s0 = s_lo; s0 < s_hi; s0 += q.ns) {
        const int ns = s_hi - s0 < q.ns ? s_hi - s0 : q.ns;
#pragma unroll 1
        for (int b = 0; b < q.nb; ++b) {
            gn_sync();                           // the zeros are written; the last stage has been read
            gn_wm_fill(xs + 2, q.chanX, q.pitch, q.bh + 4, b * q.bh - 2, T0 + o_x, L.tile, 32, 0, s0, ns, h, w, lsh);
            gn_wm_fill(as, q.chanA, q.pitch, q.bh, b * q.bh, T0 + o_dy, L.tile, CO, co0, s0, ns, h, w, lsh);
            gn_sync();
#pragma unroll 1
            for (int s = 0; s < ns; ++s)
                gn_wm_steps(acc, ap + s * 32 * q.chanA, bp + s * 32 * q.chanX, toff, q.ksteps);
        }
    }

    // write-out: acc[j][r] is output channel (r & 3) + 8 (r >> 2) + 4 half, input channel col, tap
    // wave + 4 j; registers 0..7 hold channels 0..15, registers 8..15 channels 16..31
    float *out = grad + (int64_t)rows[i] * ld_g + (c2 ? g.c2w : g.c3w) + co0 * 800;
    if constexpr (SPLIT)
        if (part) out = part + (c2 ? 0 : kGnSplitC3) + co0 * 800;
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
        gn_sync();                               // the stage, or the first half, has been read
#pragma unroll
        for (int j = 0; j < kGnWmTiles; ++j) {
            if (j >= my) continue;               // wave-uniform
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int m = (r & 3) + 8 * (r >> 2) + 4 * half;
                gn_smem[m * 800 + col * 25 + wave + 4 * j] = acc[j][8 * hf + r];
            }
        }
        gn_sync();
        for (int e = tid; e < 16 * 800; e += 256) out[hf * 16 * 800 + e] = gn_smem[e];
    }
}
