// GN-LeNet training with the weight-gradient GEMMs' batch cut over several workgroups per row
// (k_gnl_grad_wmfma<GnSplit>, k_gnl_grad_w1mfma<NT, GnSplit>, k_gnl_grad_wsum,
// niidmix_gnlenet_nll_grad_rows_mfma_split_f32).  Included by niidmix.hip after
// model_gnlenet_grad_conv1_mfma.inc; GnSplit, gn_split_range and the two kernels' split
// instantiations are in model_gnlenet_grad_mfma.inc and model_gnlenet_grad_conv1_mfma.inc.
// ----------------------------------------------------------------------------------------------
// The two GEMM kernels' grids are n_rows x 3 and n_rows workgroups, and a workgroup walks its row's
// whole batch: at few rows and long batches (100 rows of batch 128, a sample round's 10 rows, a
// centralised baseline's one row of thousands of samples) most of the card idles.  Here K is cut:
//   CH      the chunk length in samples, gn_split_chunk: a function of the shape alone
//   chunk c of a row: its samples [c CH, min(len, (c + 1) CH)) in batch order;
//           nch = max(1, ceil(len / CH)) chunks
//   nch = 1 the one workgroup writes the block into grad: the chain, and so the bits, of the
//           kernels without the cut
//   nch > 1 chunk c's workgroup runs the same K loop over its samples and writes its [32, 800]
//           or [32, Cin 25] block into slot (row, c) of the partials, which follow the activation
//           slots in the scratch; k_gnl_grad_wsum then writes ((p0 + p1) + p2) + ... into grad
// The grid is sized by ceil(b_max / CH); a workgroup whose chunk lies past its row's last returns
// at once.  Nothing here depends on n_rows or on the other rows' lengths, so a row's bits do not
// depend on how the caller cuts the row list; no atomics, no arrival counters.
// Traffic: a chunk reads CH samples' slot arrays (x2, dy2, x3, dy3, dx2, the argmax bytes, of a
// slot of 146 KiB a sample at 1 x 28 x 28 and 196 KiB at 3 x 32 x 32) and writes gn_split_floats =
// 76800 + 800 Cin floats (about 0.3 MiB) once, which the reduction reads once.
// CH per tile class (gn_mfma_ts 4 / 2), DESIGN section 5: 16 is the faster where the grid is short
// of the card; class 2 keeps 32 so that 1000 rows of batch 20, where the cut measured slower, are
// not cut
constexpr int kGnSplitCh4 = 16, kGnSplitCh2 = 32;
constexpr int kGnWsumPer = 4;                            // elements a thread of k_gnl_grad_wsum sums

// CH of a shape; 0 where the matrix-core sample pass, and so the entry, does not take it
inline int gn_split_chunk(const GnShape &g) {
    return !gn_gsm_takes(g) ? 0 : gn_mfma_ts(g) >= 4 ? kGnSplitCh4 : kGnSplitCh2;
}

// The ordered sum of a row's partial blocks.  A workgroup per (row, 256 kGnWsumPer elements of the
// partial); thread t sums elements t, t + 256, ... of its run over the chunks in ascending order,
// kGnWsumPer independent chains whose loads are in flight together.  Consecutive lanes read and
// write consecutive floats with 4-byte accesses: grad's row base need not be 16-byte aligned.
// Rows of one chunk were written by the GEMM kernels and are skipped.
__global__ __launch_bounds__(256) void k_gnl_grad_wsum(
        const int32_t *__restrict__ batch_len, int b_max, const int32_t *__restrict__ rows, int n_blk,
        const GnShape g, const GnSplit sp, float *__restrict__ grad, int64_t ld_g) {
    const int64_t i = blockIdx.x / (unsigned)n_blk;
    const int e0 = (int)(blockIdx.x % (unsigned)n_blk) * 256 * kGnWsumPer + threadIdx.x;
    const int len = lin_len(batch_len, i, b_max), nch = (len + sp.ch - 1) / sp.ch;
    if (nch <= 1) return;
    const int pb = gn_split_floats(g.Cin);
    const float *p = sp.part + i * sp.nchm * pb;
    int e[kGnWsumPer];
    float a[kGnWsumPer];
#pragma unroll
    for (int u = 0; u < kGnWsumPer; ++u) {
        e[u] = e0 + 256 * u < pb ? e0 + 256 * u : pb - 1;        // the last block's tail repeats an element
        a[u] = p[e[u]];
    }
#pragma unroll 1
    for (int c = 1; c < nch; ++c) {
        p += pb;
#pragma unroll
        for (int u = 0; u < kGnWsumPer; ++u) a[u] += p[e[u]];
    }
    float *out = grad + (int64_t)rows[i] * ld_g;
#pragma unroll
    for (int u = 0; u < kGnWsumPer; ++u) {
        if (e0 + 256 * u >= pb) continue;
        const int o = e[u] < kGnSplitC3 ? g.c2w + e[u]
                    : e[u] < kGnSplitC1 ? g.c3w + e[u] - kGnSplitC3 : g.c1w + e[u] - kGnSplitC1;
        out[o] = a[u];
    }
}
