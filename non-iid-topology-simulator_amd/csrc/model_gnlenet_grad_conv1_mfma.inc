// GN-LeNet training with conv1's weight gradient on the matrix cores (k_gnl_grad_w1mfma,
// niidmix_gnlenet_nll_grad_rows_mfma_conv1_f32).  Included by niidmix.hip after
// model_gnlenet_grad_sample_mfma.inc; it reads the scratch slots that either sample kernel left and
// uses kGnWmFloats, kGnWmFill and NIIDMIX_GN_NO_PK of model_gnlenet_grad_mfma.inc.
// ----------------------------------------------------------------------------------------------
// conv1 is followed by the 3 x 3 / 2 max-pool, and the pool's argmax depends on the output channel,
// so k_gnl_grad_conv's gather of X at the argmax positions is no GEMM operand.  The gradient is a
// GEMM once the pooled gradient dy1 (L.dx2 after gn_norm_bwd<32>(p1, ..)) is put back at full
// resolution:
//   dYf[s, oc, Y, X] = sum over the <= 4 windows (pi, pj) that cover (Y, X) and whose saved argmax
//                      (L.amax) is (Y - 2 pi) 3 + (X - 2 pj), in ascending (pi, pj): dy1[s, oc, pi, pj]
//   dW1[oc, (ci, ky, kx)] = sum_s sum_(Y, X) dYf[s, oc, Y, X] Xpad[s, ci, Y + ky - 2, X + kx - 2]
// on v_mfma_f32_32x32x2_f32:
//   M   the 32 output channels
//   N   Cin x 25 (input channel, tap) pairs in NT = ceil(Cin 25 / 32) = 1..4 tiles; a lane's column
//       n is (ci, tap) = divmod(n, 25), so B's offset ci chanX + ky pitch + kx is a per-lane
//       constant.  Lanes with n >= Cin 25 repeat column 0 and are never written
//   K   (sample in batch order, band of full-resolution rows top down, position q of the band's
//       PITCHED map), two consecutive q per MFMA (the two lane halves)
// One workgroup of 256 threads per row.  A STAGE is one sample's band of bh rows (gn_w1_geom: the
// fewest bands of equal height whose stage fits kGnWmFloats, so that two workgroups share a CU and
// one fills while the other multiplies; only rows 0 .. 2 h1 carry a gradient, the last row of an
// even H is in no window).  LDS, k_gnl_grad_wmfma's layout:
//   X    per input channel bh + 4 rows of pitch W + 2: the band's rows and two above and below (zero
//        outside the map), pixel (r, x) at r pitch + x + 2; columns 0, 1 of a row are zero and are
//        the right halo of the row before
//   dYf  per output channel bh rows of the same pitch, (r, x) at q = r pitch + x, columns W, W + 1 zero
//   dy1, amax   the pooled rows that cover the band, [32, npr, w1] floats and bytes, read coalesced
// A[m][q] = dYf[m chanA + q], B[n][q] = X[boff(n) + q]: one ds_read_b32 per lane and K-step for A,
// one per tile for B, no bounds test; chanA, chanX are odd; K per stage is bh pitch - 2 padded to
// even with a position whose dYf is zero.  The pitch stays W + 2: at W = 32 the 25 tap offsets
// ky 34 + kx fall on 13 banks (up to 3 lanes a bank), but a K-step's 1 + NT reads stand against NT
// MFMAs of 64 cycles, and the padded pitch of 37 would make K 9 % longer (DESIGN section 3).
// dYf is built by a GATHER, one lane per (oc, Y, X): no scatter, no atomics.  The zero positions
// are written once per workgroup; a stage's fill writes pixels and gradients only.
// The four waves split a stage's K-steps in four equal runs (wave w: steps [w kq, (w + 1) kq)) and
// each keeps all NT accumulator tiles in registers through the whole batch; at the end the four
// partial blocks are added through LDS in wave order, ((w0 + w1) + w2) + w3.  Every output is
// thus one chain whose order depends on the row's shape and batch length alone.
// A zero dYf position contributes 0 * x: a non-finite input pixel reaches every tap of its channel
// (in all 32 filters), where k_gnl_grad_conv's chain read the argmax positions only.
// Write-out: the row's [32, Cin 25] block at g.c1w is contiguous and goes through the then-free LDS.
struct GnW1Geom {
    int pitch, bh, nb, npr;                      // row pitch, rows per band, bands, pooled rows staged
    int chanX, chanA, ksteps, kq;                // channel strides, MFMAs per (stage, tile), per wave
};

// floats of a stage: X and dYf, 8 floats after each (a B read ends 5 past X's last channel with the
// read ahead, an A read 1 past dYf's), dy1 and the argmax bytes
__host__ __device__ __forceinline__ int gn_w1_floats(int cin, int bh, int pitch, int w1) {
    const int st = 32 * (bh / 2 + 2) * w1;
    return cin * (((bh + 4) * pitch) | 1) + 32 * ((bh * pitch) | 1) + 16 + st + (st + 3) / 4;
}

__host__ __device__ __forceinline__ GnW1Geom gn_w1_geom(int cin, int h, int w) {
    GnW1Geom q;
    const int he = 2 * gn_down(h) + 1, w1 = gn_down(w);
    q.pitch = w + 2;
    int bh = he;
    while (gn_w1_floats(cin, bh, q.pitch, w1) > kGnWmFloats) --bh;       // bh >= 7 up to 42 x 42, Cin 4
    q.nb = (he + bh - 1) / bh;
    q.bh = (he + q.nb - 1) / q.nb;
    q.npr = q.bh / 2 + 2;                        // rows (Y0 - 1) / 2 .. (Y0 + bh - 1) / 2 at most
    q.chanX = ((q.bh + 4) * q.pitch) | 1;
    q.chanA = (q.bh * q.pitch) | 1;
    q.ksteps = (q.bh * q.pitch - 1) / 2;         // K = bh * pitch - 2, rounded up to even
    q.kq = (q.ksteps + 3) / 4;
    return q;
}

// more than the write-out's 32 x Cin 25 <= 3200 floats at every shape (32 chanA >= 32 x 15 x 17)
__host__ __device__ __forceinline__ int gn_w1_lds_floats(int cin, int w, const GnW1Geom &q) {
    return gn_w1_floats(cin, q.bh, q.pitch, gn_down(w));
}

// n K-steps: ap / xp are this lane's A address and X base at the wave's first q (its row or
// column 0, its lane half), boff the offsets of the lane's NT columns
template <int NT>
__device__ __forceinline__ void gn_w1_steps(floatx16 (&acc)[NT], const float *ap, const float *xp,
                                            const int (&boff)[NT], int n) {
    const float *bt[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) bt[j] = xp + boff[j];
    // the next step's operands are read before this step's MFMAs issue; the read past the last
    // step stays inside the workgroup's LDS (gn_w1_floats) and is not used
    float a = ap[0], b[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) b[j] = bt[j][0];
#pragma unroll 1
    for (int k = 1; k <= n; ++k) {
        const float an = ap[2 * k];
        float bn[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) bn[j] = bt[j][2 * k];
#pragma unroll
        for (int j = 0; j < NT; ++j)
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b[j], acc[j], 0, 0, 0);
        a = an;
#pragma unroll
        for (int j = 0; j < NT; ++j) b[j] = bn[j];
    }
}

// Compiled without the packed fp32 VALU forms, as k_gnl_grad_wmfma is: the gather's adds are scalar
// chains of at most four terms.  k_gnl_grad_w1mfma<NT> is a workgroup per row;
// k_gnl_grad_w1mfma<NT, GnSplit> takes that one argument more and is a workgroup per (row, chunk)
// over the chunk's samples (k_gnl_grad_wmfma's rule), with the same ((w0 + w1) + w2) + w3 at its end.
template <int NT, class... SP>
__global__ __launch_bounds__(256, 2) NIIDMIX_GN_NO_PK void k_gnl_grad_w1mfma(
        const float *__restrict__ data, const int32_t *__restrict__ batch_idx,
        const int32_t *__restrict__ batch_len, int b_max, const int32_t *__restrict__ rows, int n_tiles,
        const GnShape g, const GnGradLay L, const float *__restrict__ scratch, float *__restrict__ grad,
        int64_t ld_g, const SP... sp) {
    extern __shared__ __attribute__((aligned(16))) float gn_smem[];
    constexpr bool SPLIT = sizeof...(SP) > 0;
    const int tid = threadIdx.x, wave = wave_id(), lane = tid & 63, half = lane >> 5, col = lane & 31;
    int64_t i = blockIdx.x;
    if constexpr (SPLIT) i /= (sp, ...).nchm;
    const int H = g.H, W = g.W, h1 = g.h1, w1 = g.w1, hw1 = h1 * w1, nel = g.Cin * 25;
    const GnW1Geom q = gn_w1_geom(g.Cin, H, W);
    const int len = lin_len(batch_len, i, b_max), sn = q.npr * w1;
    int s_lo = 0, s_hi = len;
    float *part = nullptr;
    if constexpr (SPLIT)                         // block-uniform, before the first barrier
        if (gn_split_range((sp, ...), i, (int)(blockIdx.x % (unsigned)(sp, ...).nchm), len, g.Cin, s_lo, s_hi, part))
            return;
    const int64_t sample = (int64_t)g.Cin * H * W;
    float *xs = gn_smem, *as = xs + g.Cin * q.chanX + 8, *dys = as + 32 * q.chanA + 8;
    unsigned char *ams = reinterpret_cast<unsigned char *>(dys + 32 * sn);

    int boff[NT];
    floatx16 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int n = col + 32 * j < nel ? col + 32 * j : 0, t = n % 25;
        boff[j] = (n / 25) * q.chanX + (t / 5) * q.pitch + t % 5;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    }
    // the zeros of the layout: once
    for (int e = tid; e < g.Cin * q.chanX + 32 * q.chanA + 16; e += 256) gn_smem[e] = 0.f;

    // the wave's run of K-steps, and the gather's first (oc, r, x) and its stride of 256 elements
    const int k0 = wave * q.kq, nk = (k0 + q.kq < q.ksteps ? k0 + q.kq : q.ksteps) - k0;
    const float *ap = as + col * q.chanA + half + 2 * k0, *xp = xs + half + 2 * k0;
    const int gx0 = tid % W, gr0 = (tid / W) % q.bh, go0 = (tid / W) / q.bh;
    const int gdx = 256 % W, gdr = 256 / W;
    const float *T0 = scratch + i * n_tiles * L.tile;        // the row's first slot
#pragma unroll 1
    for (int s = s_lo; s < s_hi; ++s) {
        // sample s lives in tile s / kGnTS of the row, at place s % kGnTS
        const float *T = T0 + (int64_t)(s / kGnTS) * L.tile;
        const float *dy1 = T + L.dx2 + (s % kGnTS) * 32 * hw1;
        const unsigned char *am = reinterpret_cast<const unsigned char *>(T + L.amax) + (s % kGnTS) * 32 * hw1;
        const float *xin = data + (int64_t)batch_idx[i * b_max + s] * sample;
#pragma unroll 1
        for (int b = 0; b < q.nb; ++b) {
            const int Y0 = b * q.bh;
            // the pooled rows whose windows reach the band
            const int pr0 = Y0 < 2 ? 0 : (Y0 - 1) / 2;
            const int pr1 = (Y0 + q.bh - 1) / 2 < h1 - 1 ? (Y0 + q.bh - 1) / 2 : h1 - 1;
            const int np = (pr1 - pr0 + 1) * w1, nxr = g.Cin * (q.bh + 4);
            gn_sync();                           // the zeros are written; the last stage has been read
            // dy1 and the argmax: a wave per output channel, 8 channels' loads in flight per lane
            for (int k = lane; k < np; k += 64) {
                float v[8];
                unsigned char a[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    v[u] = dy1[(wave + 4 * u) * hw1 + pr0 * w1 + k];
                    a[u] = am[(wave + 4 * u) * hw1 + pr0 * w1 + k];
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    dys[(wave + 4 * u) * sn + k] = v[u];
                    ams[(wave + 4 * u) * sn + k] = a[u];
                }
            }
            // X: a wave per (channel, row) of the band and its halo rows, a lane per pixel (W <= 64),
            // kGnWmFill rows' loads in flight
#pragma unroll 1
            for (int it0 = wave; it0 < nxr; it0 += 4 * kGnWmFill) {
                float v[kGnWmFill];
#pragma unroll
                for (int u = 0; u < kGnWmFill; ++u) {
                    const int it = it0 + 4 * u, ci = it / (q.bh + 4), y = Y0 - 2 + it % (q.bh + 4);
                    const bool in = it < nxr && lane < W && (unsigned)y < (unsigned)H;
                    v[u] = in ? xin[(ci * H + y) * W + lane] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < kGnWmFill; ++u) {
                    const int it = it0 + 4 * u, ci = it / (q.bh + 4), r = it % (q.bh + 4);
                    if (it < nxr && lane < W) xs[ci * q.chanX + r * q.pitch + lane + 2] = v[u];
                }
            }
            gn_sync();
            // dYf: a lane per (oc, r, x), elements tid, tid + 256, ... of [32, bh, W]
            for (int oc = go0, r = gr0, x = gx0; oc < 32;) {
                const int Y = Y0 + r;
                // the windows (i0 or i0 + 1, j0 or j0 + 1) that exist and cover (Y, x): all four are
                // read (the second row and column clamped into the stage), then added in ascending order
                const int i0 = Y < 2 ? 0 : (Y - 1) >> 1, i1 = (Y >> 1) < h1 - 1 ? (Y >> 1) : h1 - 1;
                const int j0 = x < 2 ? 0 : (x - 1) >> 1, j1 = (x >> 1) < w1 - 1 ? (x >> 1) : w1 - 1;
                const int ia = i0 < pr1 ? i0 : pr1, ib = i0 + 1 < pr1 ? i0 + 1 : pr1;
                const int ja = j0 < w1 - 1 ? j0 : w1 - 1, jb = j0 + 1 < w1 - 1 ? j0 + 1 : w1 - 1;
                const int e00 = oc * sn + (ia - pr0) * w1 + ja, e10 = oc * sn + (ib - pr0) * w1 + ja;
                const int e01 = e00 + jb - ja, e11 = e10 + jb - ja;
                const int c00 = ams[e00], c01 = ams[e01], c10 = ams[e10], c11 = ams[e11];
                const float d00 = dys[e00], d01 = dys[e01], d10 = dys[e10], d11 = dys[e11];
                const int t0 = (Y - 2 * i0) * 3 + (x - 2 * j0);      // the argmax that names (Y, x) in window (i0, j0)
                float a = 0.f;
                if (i0 <= i1 && j0 <= j1 && c00 == t0) a += d00;
                if (i0 <= i1 && j0 + 1 <= j1 && c01 == t0 - 2) a += d01;
                if (i0 + 1 <= i1 && j0 <= j1 && c10 == t0 - 6) a += d10;
                if (i0 + 1 <= i1 && j0 + 1 <= j1 && c11 == t0 - 8) a += d11;
                as[oc * q.chanA + r * q.pitch + x] = a;
                x += gdx;
                r += gdr;
                if (x >= W) { x -= W; ++r; }
                while (r >= q.bh) { r -= q.bh; ++oc; }
            }
            gn_sync();
            if (nk > 0) gn_w1_steps<NT>(acc, ap, xp, boff, nk);      // wave-uniform
        }
    }

    // the four partial blocks, added in wave order in LDS: acc[j][r] is output channel
    // (r & 3) + 8 (r >> 2) + 4 half, column col + 32 j
#pragma unroll 1
    for (int wv = 0; wv < 4; ++wv) {
        gn_sync();                               // the last stage has been read; wave wv - 1 has added
        if (wave != wv) continue;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            if (col + 32 * j >= nel) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float *p = gn_smem + ((r & 3) + 8 * (r >> 2) + 4 * half) * nel + col + 32 * j;
                *p = wv == 0 ? acc[j][r] : *p + acc[j][r];
            }
        }
    }
    gn_sync();
    float *out = grad + (int64_t)rows[i] * ld_g + g.c1w;
    if constexpr (SPLIT)
        if (part) out = part + kGnSplitC1;
    for (int e = tid; e < 32 * nel; e += 256) out[e] = gn_smem[e];
}
