// Training batches drawn on the device (niidmix_draw_batches_i32; --device-sampling) and the cached
// mode's whole-epoch permutations (niidmix_epoch_perm_i32, niidmix_take_batches_i32;
// --device-sampling-cached), and torch's own permutations for the same cache
// (niidmix_torch_randperm_i32; --device-sampling-torch-stream, at the end of the file).  Included by
// niidmix.hip; the host restatement of both streams is niidmix/sampling.py.
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
//                     leave at once (draw_sort_wave)
//   longer            the composites in LDS, four per Philox call, padded with all-ones to the
//                     next power of two (draw_fill_lds); a bitonic network with a barrier per
//                     stage, a thread taking kDrawUnroll disjoint comparators per pass (all loads,
//                     then all stores; draw_network_lds)
// A segment longer than kDrawMaxLen is clamped to it (the Python side refuses such a node list),
// a cursor outside the segment gives an empty batch: nothing is read or written out of range
// whatever the device arrays hold.
// The cached mode sorts once per epoch and keeps the order in HBM (k_epoch_perm_*), then slices it
// every round (k_take_batches).  Segments up to kDrawMaxLen take the two paths above and write
// the order straight out.  A longer one is one bitonic network over pow2(len) composites in a
// scratch of 8 B each, a workgroup per chunk of kDrawMaxLen of them:
//   k_epoch_perm_chunks  generates the chunk in LDS and runs the network's levels k <= kDrawMaxLen
//                        on it (draw_network_lds: a comparator's direction comes from the GLOBAL
//                        position, base + lo, so odd chunks come out descending as the network
//                        wants), then stores it
//   k_epoch_perm_global  one stage (k, j) with j >= kDrawMaxLen: a thread exchanges two adjacent
//                        composites with the two at distance j, 16-B loads and stores
//   k_epoch_perm_finish  the stages j < kDrawMaxLen of level k, in LDS, a chunk per workgroup; the
//                        job's last level (k = pow2(len)) writes the order's low words to perm
//                        instead of the scratch
// Every stage reads what the previous launch wrote and every word has one writer, so the result
// does not depend on scheduling.  Jobs of one call may differ in length: a workgroup beyond its
// job's padded length, or at a level above it, leaves at once.
constexpr int kDrawMaxLen = 8192;        // composites of 8 B in 64 KiB of LDS
constexpr int kDrawThreads = 256;
constexpr int kDrawUnroll = 4;
constexpr int kEpochPermMaxLen = 1 << 20;   // 7 levels above the chunks: 28 global + 7 LDS passes

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

// A segment of len <= 64 sorted by one wave (tid < 64): returns entry `tid` of the ascending order
// of the composites (all-ones from len on).
__device__ __forceinline__ uint64_t draw_sort_wave(uint32_t seed, uint32_t k1, uint32_t e, int len, int tid) {
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
    return v;
}

// The composites of positions base .. base + n - 1 of a segment of `len` samples into s[0 .. n):
// n and base multiples of 4, four positions per Philox call, all-ones from len on.
__device__ __forceinline__ void draw_fill_lds(uint64_t *s, int n, int base, int len, uint32_t seed,
                                              uint32_t k1, uint32_t e, int tid) {
    for (int q = tid; q < n / 4; q += kDrawThreads) {
        const Philox4 p = philox4x32_10((uint32_t)(base / 4 + q), e, 0u, 0u, seed, k1);
#pragma unroll
        for (int w = 0; w < 4; ++w) s[4 * q + w] = draw_composite(p.w[w], base + 4 * q + w, len);
    }
}

// The levels k_lo .. k_hi (powers of two) of an ascending bitonic network on the n composites
// (a power of two >= 2) that s holds, which stand at positions base .. base + n - 1 of the whole
// network (base a multiple of n): the stages j < n of each level, a barrier after each.  With
// base 0, k_lo 2 and k_hi n it sorts s; a chunk of a longer network takes its levels in pieces.
// The caller has a barrier between its writes of s and the call.
__device__ __forceinline__ void draw_network_lds(uint64_t *s, int n, int base, int k_lo, int k_hi, int tid) {
    const int half = n / 2;
    for (int k = k_lo; k <= k_hi; k <<= 1) {
        for (int j = k >> 1 < half ? k >> 1 : half; j > 0; j >>= 1) {
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
                    if (c < half && (a[u] > b[u]) == (((base | lo[u]) & k) == 0)) {
                        s[lo[u]] = b[u];
                        s[lo[u] | j] = a[u];
                    }
                }
            }
            __syncthreads();
        }
    }
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
        const uint64_t v = draw_sort_wave(seed, k1, e, len, tid);
        if (tid >= cur && tid < cur + n) out[tid - cur] = start + (int32_t)(uint32_t)v;
        return;
    }

    int n_pad = 128;
    while (n_pad < len) n_pad <<= 1;                         // <= kDrawMaxLen
    draw_fill_lds(s, n_pad, 0, len, seed, k1, e, tid);
    __syncthreads();
    draw_network_lds(s, n_pad, 0, 2, n_pad, tid);
    for (int t = tid; t < n; t += kDrawThreads) out[t] = start + (int32_t)(uint32_t)s[cur + t];
}

// ----------------------------------------------------------------------------------------------
// The cached mode.  What every k_epoch_perm_* kernel knows of job `job`: its clamped length, the
// padded length of its network and where its order goes; len 0 says "skip the job" (an empty
// segment, or a stretch [perm_off, perm_off + len) that does not lie inside perm).
struct EpochJob {
    int len, n_pad;
    int64_t off;
};

__device__ __forceinline__ EpochJob epoch_job(const int32_t *seg_len, const int64_t *perm_off, int64_t job,
                                              int max_len, int64_t perm_len) {
    EpochJob J;
    const int len = seg_len[job];
    J.len = len < 0 ? 0 : len > max_len ? max_len : len;
    J.off = perm_off[job];
    if (J.off < 0 || J.off > perm_len - J.len) J.len = 0;
    J.n_pad = kDrawMaxLen;
    while (J.n_pad < J.len) J.n_pad <<= 1;                   // <= pow2(max_len) <= kEpochPermMaxLen
    return J;
}

// grid (n_jobs, chunks of the longest padded length).  A segment up to kDrawMaxLen: chunk 0 sorts
// it as k_draw_batches does and writes its order; a longer one: every chunk inside the padded
// length is generated, sorted in the direction the whole network wants and stored to the scratch
// (job_stride composites per job).
__global__ __launch_bounds__(kDrawThreads) void k_epoch_perm_chunks(
        uint32_t seed, const int32_t *__restrict__ rank, const int32_t *__restrict__ seg_len,
        const int32_t *__restrict__ epoch, const int64_t *__restrict__ perm_off, int max_len,
        int32_t *__restrict__ perm, int64_t perm_len, uint64_t *__restrict__ scratch, int64_t job_stride) {
    __shared__ uint64_t s[kDrawMaxLen];
    const int64_t job = blockIdx.x;
    const int tid = threadIdx.x, base = blockIdx.y * kDrawMaxLen;
    const EpochJob J = epoch_job(seg_len, perm_off, job, max_len, perm_len);
    if (J.len == 0 || base >= J.n_pad) return;               // uniform over the workgroup
    if (J.len <= kDrawMaxLen && base != 0) return;
    const uint32_t k1 = (uint32_t)rank[job], e = (uint32_t)epoch[job];
    int32_t *out = perm + J.off;

    if (J.len <= 64) {
        if (tid >= 64) return;
        const uint64_t v = draw_sort_wave(seed, k1, e, J.len, tid);
        if (tid < J.len) out[tid] = (int32_t)(uint32_t)v;
        return;
    }
    if (J.len <= kDrawMaxLen) {
        int n_pad = 128;
        while (n_pad < J.len) n_pad <<= 1;
        draw_fill_lds(s, n_pad, 0, J.len, seed, k1, e, tid);
        __syncthreads();
        draw_network_lds(s, n_pad, 0, 2, n_pad, tid);
        for (int t = tid; t < J.len; t += kDrawThreads) out[t] = (int32_t)(uint32_t)s[t];
        return;
    }
    draw_fill_lds(s, kDrawMaxLen, base, J.len, seed, k1, e, tid);
    __syncthreads();
    draw_network_lds(s, kDrawMaxLen, base, 2, kDrawMaxLen, tid);
    ulonglong2 *dst = reinterpret_cast<ulonglong2 *>(scratch + job * job_stride + base);
    for (int t = tid; t < kDrawMaxLen / 2; t += kDrawThreads) dst[t] = make_ulonglong2(s[2 * t], s[2 * t + 1]);
}

// Stage (k, j), j >= kDrawMaxLen, of the long jobs' networks in the scratch: grid (n_jobs, pairs of
// comparators of the longest padded length / kDrawThreads); a thread takes the comparators 2m and
// 2m + 1, whose lower ends are adjacent (j is even), as one 16-B exchange.
__global__ __launch_bounds__(kDrawThreads) void k_epoch_perm_global(
        const int32_t *__restrict__ seg_len, const int64_t *__restrict__ perm_off, int max_len,
        int64_t perm_len, uint64_t *__restrict__ scratch, int64_t job_stride, int k, int j) {
    const int64_t job = blockIdx.x;
    const EpochJob J = epoch_job(seg_len, perm_off, job, max_len, perm_len);
    const int c = 2 * (blockIdx.y * kDrawThreads + threadIdx.x);
    if (J.len <= kDrawMaxLen || k > J.n_pad || c >= J.n_pad / 2) return;
    const int lo = ((c & ~(j - 1)) << 1) | (c & (j - 1));
    uint64_t *g = scratch + job * job_stride;
    ulonglong2 a = *reinterpret_cast<ulonglong2 *>(g + lo), b = *reinterpret_cast<ulonglong2 *>(g + (lo | j));
    const bool up = (lo & k) == 0;
    const bool sx = (a.x > b.x) == up, sy = (a.y > b.y) == up;
    if (sx || sy) {
        *reinterpret_cast<ulonglong2 *>(g + lo) = make_ulonglong2(sx ? b.x : a.x, sy ? b.y : a.y);
        *reinterpret_cast<ulonglong2 *>(g + (lo | j)) = make_ulonglong2(sx ? a.x : b.x, sy ? a.y : b.y);
    }
}

// The stages j < kDrawMaxLen of level k, a chunk per workgroup (grid as k_epoch_perm_chunks).  A
// job whose network ends at this level gets its order written to perm; the others go on in the
// scratch.
__global__ __launch_bounds__(kDrawThreads) void k_epoch_perm_finish(
        const int32_t *__restrict__ seg_len, const int64_t *__restrict__ perm_off, int max_len,
        int32_t *__restrict__ perm, int64_t perm_len, uint64_t *__restrict__ scratch, int64_t job_stride,
        int k) {
    __shared__ uint64_t s[kDrawMaxLen];
    const int64_t job = blockIdx.x;
    const int tid = threadIdx.x, base = blockIdx.y * kDrawMaxLen;
    const EpochJob J = epoch_job(seg_len, perm_off, job, max_len, perm_len);
    if (J.len <= kDrawMaxLen || k > J.n_pad || base >= J.n_pad) return;      // uniform
    ulonglong2 *g = reinterpret_cast<ulonglong2 *>(scratch + job * job_stride + base);
    for (int t = tid; t < kDrawMaxLen / 2; t += kDrawThreads) {
        const ulonglong2 v = g[t];
        s[2 * t] = v.x;
        s[2 * t + 1] = v.y;
    }
    __syncthreads();
    draw_network_lds(s, kDrawMaxLen, base, k, k, tid);
    if (k == J.n_pad) {                  // ascending over the whole network: the padding is last
        int32_t *out = perm + J.off + base;
        const int n = J.len - base < kDrawMaxLen ? J.len - base : kDrawMaxLen;
        for (int t = tid; t < n; t += kDrawThreads) out[t] = (int32_t)(uint32_t)s[t];
    } else {
        for (int t = tid; t < kDrawMaxLen / 2; t += kDrawThreads) g[t] = make_ulonglong2(s[2 * t], s[2 * t + 1]);
    }
}

// The round's slice of the cached orders: grid (n_jobs, tiles of kDrawThreads batch slots).  A
// cursor outside the segment, or a stretch outside perm, gives an empty batch.
__global__ __launch_bounds__(kDrawThreads) void k_take_batches(
        const int32_t *__restrict__ perm, int64_t perm_len, const int64_t *__restrict__ perm_off,
        const int32_t *__restrict__ seg_start, const int32_t *__restrict__ seg_len,
        const int32_t *__restrict__ cursor, int b_max, int32_t *__restrict__ batch_idx,
        int32_t *__restrict__ batch_len) {
    const int64_t job = blockIdx.x;
    const int t = blockIdx.y * kDrawThreads + threadIdx.x;
    const int len = seg_len[job], cur = cursor[job];
    const int64_t off = perm_off[job];
    int n = len <= 0 || cur < 0 || cur >= len || off < 0 || off > perm_len - len ? 0 : len - cur;
    n = n > b_max ? b_max : n;
    if (t == 0) batch_len[job] = n;
    if (t < n) batch_idx[job * b_max + t] = seg_start[job] + perm[off + cur + t];
}

// ----------------------------------------------------------------------------------------------
// torch's stream (--device-sampling-torch-stream): the permutation torch.randperm(len, generator=g)
// gives on the CPU after g.manual_seed(s), for the cache k_take_batches slices.  ATen seeds MT19937
// with the low 32 bits of s (init_genrand) and runs
//     for i in 0 .. len-2:  z = next_u32 % (len - i);  swap(a[i], a[i + z])
// on a = 0 .. len-1.  k_torch_randperm: one workgroup per job, everything in dynamic LDS -- the
// positions as uint16 (len <= 65536), the 624 state words, one block of 624 reduced z.  Seeding is a
// serial chain (one lane).  Per block of 624 draws: the twist in three stretches of (at most) 227
// words, each reading what the one before wrote (all loads, a barrier, all stores); tempering and
// the reduction modulo len - i by all lanes; then one lane walks the block's swaps, eight z per
// 16-B load.  The result goes out as int32 with all lanes.  Only the walk is serial in len.
constexpr int kTorchPermMaxLen = 65536;     // positions as uint16: 128 KiB of LDS
constexpr int kMtN = 624, kMtM = 397;
static_assert(kDrawThreads >= kMtN - kMtM && kMtN - 2 * (kMtN - kMtM) <= kDrawThreads && kMtN % 8 == 0,
              "a twist stretch is one word per thread; the walk loads eight z at a time");

// bytes of dynamic LDS for jobs of up to max_len samples: positions | state | z, each 16-B aligned
__host__ __device__ constexpr size_t torch_perm_pos_bytes(int max_len) {
    return ((size_t)max_len * 2 + 15) / 16 * 16;
}
__host__ __device__ constexpr size_t torch_perm_lds_bytes(int max_len) {
    return torch_perm_pos_bytes(max_len) + kMtN * 4 + kMtN * 2;
}

// One regeneration of the state (genrand's next_state), in place, by the whole workgroup; ends
// with a barrier.
__device__ __forceinline__ void mt_twist(uint32_t *mt, int tid) {
    constexpr int kStretch = kMtN - kMtM;                    // 227
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        const int k = s * kStretch + tid, end = s < 2 ? (s + 1) * kStretch : kMtN;
        uint32_t v = 0;
        if (k < end) {
            // word k + 397 (mod 624) is old in the first stretch and new afterwards; word k + 1 is
            // old except for k = 623, whose successor is the new word 0
            const uint32_t u = mt[k], w = mt[k + 1 == kMtN ? 0 : k + 1];
            const uint32_t y = (u & 0x80000000u) | (w & 0x7fffffffu);
            v = mt[k < kStretch ? k + kMtM : k - kStretch] ^ (y >> 1) ^ (w & 1u ? 0x9908b0dfu : 0u);
        }
        __syncthreads();                                     // word k + 1 is read before it is written
        if (k < end) mt[k] = v;
        __syncthreads();
    }
}

__global__ __launch_bounds__(kDrawThreads) void k_torch_randperm(
        const int32_t *__restrict__ seed_lo, const int32_t *__restrict__ seg_len,
        const int64_t *__restrict__ perm_off, int max_len, int32_t *__restrict__ perm, int64_t perm_len) {
    extern __shared__ __attribute__((aligned(16))) unsigned char torch_perm_lds[];
    const int64_t job = blockIdx.x;
    const int tid = threadIdx.x;
    const int n = seg_len[job];
    const int64_t off = perm_off[job];
    if (n < 1 || n > max_len || off < 0 || off > perm_len - n) return;      // uniform: the job is skipped
    uint16_t *a = reinterpret_cast<uint16_t *>(torch_perm_lds);
    uint32_t *mt = reinterpret_cast<uint32_t *>(torch_perm_lds + torch_perm_pos_bytes(max_len));
    uint16_t *z = reinterpret_cast<uint16_t *>(mt + kMtN);

    for (int t = tid; t < n; t += kDrawThreads) a[t] = (uint16_t)t;
    if (tid == 0) {                                          // init_genrand
        uint32_t s = (uint32_t)seed_lo[job];
        mt[0] = s;
        for (uint32_t j = 1; j < (uint32_t)kMtN; ++j) {
            s = 1812433253u * (s ^ (s >> 30)) + j;
            mt[j] = s;
        }
    }
    __syncthreads();
    for (int base = 0; base < n - 1; base += kMtN) {         // draws base .. base + cnt - 1
        mt_twist(mt, tid);
        const int cnt = n - 1 - base < kMtN ? n - 1 - base : kMtN;
        for (int k = tid; k < cnt; k += kDrawThreads) {
            uint32_t y = mt[k];
            y ^= y >> 11;
            y ^= (y << 7) & 0x9d2c5680u;
            y ^= (y << 15) & 0xefc60000u;
            y ^= y >> 18;
            z[k] = (uint16_t)(y % (uint32_t)(n - (base + k)));          // < n - i <= 65536, n - i >= 2
        }
        __syncthreads();
        if (tid == 0) {
            for (int k0 = 0; k0 < cnt; k0 += 8) {
                const uint4 q = *reinterpret_cast<const uint4 *>(z + k0);
                const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    if (k0 + u < cnt) {
                        const int i = base + k0 + u, t = i + (int)((w[u >> 1] >> (16 * (u & 1))) & 0xffffu);
                        const uint16_t x = a[i], y = a[t];                 // t <= n - 1
                        a[i] = y;
                        a[t] = x;
                    }
                }
            }
        }
        __syncthreads();
    }
    int32_t *out = perm + off;
    for (int t = tid; t < n; t += kDrawThreads) out[t] = (int32_t)a[t];
}
