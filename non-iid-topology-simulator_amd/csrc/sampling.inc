// Training batches drawn on the device (niidmix_draw_batches_i32; --device-sampling).  Included
// by niidmix.hip; the host restatement of the same stream is niidmix/sampling.py.
// ----------------------------------------------------------------------------------------------
// The stream, in integers only.  Position i of a segment of `len` samples, for the node of rank r
// in epoch e under the run seed s, gets the 32-bit key
//     k_i = word (i & 3) of Philox4x32-10(counter (i >> 2, e, 0, 0), key (s, r)),
// and epoch e visits the positions in ascending order of the composites (k_i << 32) | i, which are
// distinct by construction.  A batch is b_max consecutive entries of that order from `cursor` on,
// fewer at the segment's end.
// k_draw_batches: one workgroup per job, stateless -- every call sorts the job's whole segment
// again (segments are tens to a few thousand samples), so nothing but (epoch, cursor) lives
// between rounds, and that on the host.
//   up to 64 samples  wave 0 alone, a composite per lane, a bitonic network of __shfl_xor
//                     exchanges over the next power of two: no LDS, no barrier; the other waves
//                     leave at once
//   longer            the composites in LDS, four per Philox call, padded with all-ones to the
//                     next power of two; a bitonic network with a barrier per stage, a thread
//                     taking kDrawUnroll disjoint comparators per pass (all loads, then all
//                     stores)
// A segment longer than kDrawMaxLen is clamped to it (the Python side refuses such a node list),
// a cursor outside the segment gives an empty batch: nothing is read or written out of range
// whatever the device arrays hold.
constexpr int kDrawMaxLen = 8192;        // composites of 8 B in 64 KiB of LDS
constexpr int kDrawThreads = 256;
constexpr int kDrawUnroll = 4;

struct Philox4 {
    uint32_t w[4];
};

__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                                 uint32_t k0, uint32_t k1) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(M0, c0), l0 = M0 * c0;
        const uint32_t h1 = __umulhi(M1, c2), l1 = M1 * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += W0;                         // the key of the next round
        k1 += W1;
    }
    return Philox4{{c0, c1, c2, c3}};
}

__device__ __forceinline__ uint64_t draw_composite(uint32_t key, int i, int len) {
    return i < len ? ((uint64_t)key << 32) | (uint32_t)i : ~0ull;
}

__global__ __launch_bounds__(kDrawThreads) void k_draw_batches(
        uint32_t seed, const int32_t *__restrict__ rank, const int32_t *__restrict__ seg_start,
        const int32_t *__restrict__ seg_len, const int32_t *__restrict__ epoch,
        const int32_t *__restrict__ cursor, int b_max, int32_t *__restrict__ batch_idx,
        int32_t *__restrict__ batch_len) {
    __shared__ uint64_t s[kDrawMaxLen];
    const int64_t job = blockIdx.x;
    const int tid = threadIdx.x;
    int len = seg_len[job];
    len = len < 0 ? 0 : len > kDrawMaxLen ? kDrawMaxLen : len;
    const int cur = cursor[job];
    int n = cur < 0 || cur >= len ? 0 : len - cur;          // this batch's entries
    n = n > b_max ? b_max : n;
    const uint32_t k1 = (uint32_t)rank[job], e = (uint32_t)epoch[job];
    const int32_t start = seg_start[job];
    int32_t *out = batch_idx + job * b_max;
    if (tid == 0) batch_len[job] = n;
    if (n == 0) return;                                      // uniform over the workgroup

    if (len <= 64) {                                         // uniform too: the one-wave path
        if (tid >= 64) return;
        int n_pad = 1;
        while (n_pad < len) n_pad <<= 1;
        const Philox4 p = philox4x32_10((uint32_t)(tid >> 2), e, 0u, 0u, seed, k1);
        const uint32_t key = tid & 2 ? (tid & 1 ? p.w[3] : p.w[2]) : (tid & 1 ? p.w[1] : p.w[0]);
        uint64_t v = draw_composite(key, tid, len);
        for (int k = 2; k <= n_pad; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                const uint64_t o = __shfl_xor((unsigned long long)v, j);
                // the lower lane of a pair keeps the smaller value in an ascending block
                const bool keep_min = ((tid & j) == 0) == ((tid & k) == 0);
                v = keep_min ? (v < o ? v : o) : (v < o ? o : v);
            }
        }
        if (tid >= cur && tid < cur + n) out[tid - cur] = start + (int32_t)(uint32_t)v;
        return;
    }

    int n_pad = 128;
    while (n_pad < len) n_pad <<= 1;                         // <= kDrawMaxLen
    for (int q = tid; q < n_pad / 4; q += kDrawThreads) {
        const Philox4 p = philox4x32_10((uint32_t)q, e, 0u, 0u, seed, k1);
#pragma unroll
        for (int w = 0; w < 4; ++w) s[4 * q + w] = draw_composite(p.w[w], 4 * q + w, len);
    }
    __syncthreads();
    const int half = n_pad / 2;
    for (int k = 2; k <= n_pad; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int c0 = tid; c0 < half; c0 += kDrawThreads * kDrawUnroll) {
                uint64_t a[kDrawUnroll], b[kDrawUnroll];
                int lo[kDrawUnroll];
#pragma unroll
                for (int u = 0; u < kDrawUnroll; ++u) {
                    const int c = c0 + u * kDrawThreads;
                    // comparator c of the stage: its lower index has bit j clear
                    lo[u] = ((c & ~(j - 1)) << 1) | (c & (j - 1));
                    if (c < half) {
                        a[u] = s[lo[u]];
                        b[u] = s[lo[u] | j];
                    }
                }
#pragma unroll
                for (int u = 0; u < kDrawUnroll; ++u) {
                    const int c = c0 + u * kDrawThreads;
                    if (c < half && (a[u] > b[u]) == ((lo[u] & k) == 0)) {
                        s[lo[u]] = b[u];
                        s[lo[u] | j] = a[u];
                    }
                }
            }
            __syncthreads();
        }
    }
    for (int t = tid; t < n; t += kDrawThreads) out[t] = start + (int32_t)(uint32_t)s[cur + t];
}
