// Lloyd k-means for eval/kmeans.py (kmeans_ari): assignment on the fp32 matrix pipe, a deterministic full-scale centre
// update and faiss's empty-cluster split.
//
//   * km_assign_kernel / km_assign_wide_kernel: nearest centre of every row.  They read the tile images of
//     tdr_pack_rows_f32 (D <= 256) / tdr_pack_rows_wide_f32 (D > 256) for the rows AND the centres, form every candidate
//     with the exact kNN kernels' expansion c = fma(-2, x.y, ||x||^2 + ||y||^2) on one k-ordered v_mfma_f32_32x32x2f32
//     chain, and keep the minimum of the kNN's 64-bit (distance, index) key -- so label and distance are the bits of
//     tdr_knn_packed_f32 / tdr_knn_wide_f32 with k = 1, metric sqeuclidean, ties to the lower centre index.  There is no
//     top-k list: a lane keeps one key, filtered by one compare per candidate.  The centres stream through a
//     double-buffered LDS ring, so any number of centres works.  Each workgroup leaves the float64 sum of its rows'
//     distances (fixed order); km_fold_kernel folds those partials in workgroup order.
//   * Update: the rows are sorted stably by label with a counting sort (per-block histogram H[label][block] by integer
//     atomics, one exclusive scan, a per-block stable scatter), so each cluster is a run of its members in ascending row
//     order.  Clusters are cut into segments of KM_SEG rows; a workgroup sums one (segment, 64-column block) in float64
//     in row order.  A cluster of one segment writes its mean directly, longer ones leave partials that
//     km_finalize_kernel folds in segment order.  O(N D) bytes per step, no float atomics.
//   * km_split_kernel: faiss's split_clusters (clustering/Clustering.cpp) with a counter-based draw.
#include "tdr_common.h"

namespace tdr {
namespace km {

constexpr int TILE_ROWS = 32;
constexpr uint64_t KEY_SENTINEL = 0xFF800000FFFFFFFFull;  // (+inf, 0xffffffff): above every real candidate
constexpr int SEG = 256;            // rows of one update segment
constexpr int SCAN_THREADS = 1024;
constexpr int64_t HIST_BUDGET = 1 << 20;  // entries of H = labels x row blocks
constexpr int WIDE_TG = 4;          // wide kernel: centre tiles accumulated together (one per wavefront to stage)
constexpr int WIDE_KC = 4;          // wide kernel: 8-dim blocks per K step

typedef __attribute__((address_space(1))) const void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

__host__ __device__ __forceinline__ int64_t tile_stride_floats(int kq) { return (int64_t)kq * 256 + 64; }

struct AssignParams {
    const float* xp;   // packed rows
    int64_t n;
    const float* cp;   // packed centres
    int64_t c;
    int n_ctiles;
    int kq;            // wide kernel: 8-dim blocks per image (run-time)
    int32_t* labels;
    float* dist;
    double* partial;   // one float64 sum per workgroup
};

// One finished 32 x 32 block: 16 candidates per lane (centre rows (r&3) + 8*(r>>2) + 4*h of tile T), the kNN kernels'
// form_part expansion, filtered by one compare against the lane's best distance; survivors compared by the full key.
__device__ __forceinline__ void fold_tile(const f32x16& acc, const float* ynp, float xn, int T, int64_t c, int h,
                                          uint64_t& best, float& best_d) {
    float dv[16];
    float m = __builtin_inff();
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 y4 = *reinterpret_cast<const f32x4*>(ynp + 8 * g + 4 * h);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int r = 4 * g + e;
            dv[r] = __builtin_fmaf(-2.0f, acc[r], __fadd_rn(xn, y4[e]));
            m = fminf(m, dv[r]);
        }
    }
    if (m <= best_d) {  // rare after the first tiles
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t j = (int64_t)T * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (j < c && dv[r] <= best_d) {
                const uint64_t key = mkkey(dv[r], (uint32_t)j);
                if (key < best) { best = key; best_d = u2f((uint32_t)(key >> 32)); }
            }
        }
    }
}

// Merge the two half-lanes of a query (rows 4h.. of every tile), write label / distance, and leave the workgroup's
// float64 sum of distances: lanes in a fixed shuffle tree, then waves 0..3 in order.
__device__ __forceinline__ void emit(const AssignParams& P, uint64_t best, int64_t qrow, bool valid, int lane, int wave) {
    __shared__ double wsum[4];
    const uint32_t lo = (uint32_t)best, hi = (uint32_t)(best >> 32);
    const uint32_t olo = (uint32_t)__shfl_xor((int)lo, 32, 64), ohi = (uint32_t)__shfl_xor((int)hi, 32, 64);
    const uint64_t other = ((uint64_t)ohi << 32) | olo;
    if (other < best) best = other;
    double s = 0.0;
    if (valid) {
        const float d = u2f((uint32_t)(best >> 32));
        if (lane < 32) {
            P.labels[qrow] = (int32_t)(uint32_t)(best & 0xffffffffu);
            P.dist[qrow] = d;
            s = (double)d;
        }
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) wsum[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) P.partial[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// D <= 256: a wavefront owns 32 rows whose feature blocks sit in VGPRs (MFMA B operand) for the whole scan; centre tiles
// (A operand) are staged by LDS-DMA, one tile ahead.
template <int KQ>
__global__ __launch_bounds__(256, 2) void km_assign_kernel(const AssignParams P) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    constexpr int NW = 4;
    constexpr int IMG_F = KQ * 256;
    constexpr int TILE_F = IMG_F + 64;
    float* tile0 = reinterpret_cast<float*>(smem_raw);
    float* tile1 = tile0 + IMG_F;
    float* nring = tile1 + IMG_F;  // [2][64]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane & 31, h = lane >> 5;
    const int64_t n_qtiles = (P.n + 31) / 32;
    const int64_t qt = (int64_t)blockIdx.x * NW + wave;
    const bool active = qt < n_qtiles;
    float b[4 * KQ];
    float xn = 0.f;
    if (active) {
        const float* qimg = P.xp + (size_t)qt * TILE_F;
#pragma unroll
        for (int t = 0; t < KQ; ++t) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(qimg + t * 256 + lane * 4);
            b[4 * t + 0] = v[0]; b[4 * t + 1] = v[1]; b[4 * t + 2] = v[2]; b[4 * t + 3] = v[3];
        }
        xn = qimg[IMG_F + q];
    } else {
#pragma unroll
        for (int t = 0; t < 4 * KQ; ++t) b[t] = 0.f;
    }
    auto stage = [&](int T) {
        const float* src = P.cp + (size_t)T * TILE_F;
        float* dst = (T & 1) ? tile1 : tile0;
#pragma unroll
        for (int t = 0; t < KQ; t += NW) {
            const int blk = t + wave;
            if (blk < KQ)
                __builtin_amdgcn_global_load_lds((gptr_t)(src + blk * 256 + lane * 4), (lptr_t)(dst + blk * 256), 16, 0, 0);
        }
        if (wave == NW - 1)
            __builtin_amdgcn_global_load_lds((gptr_t)(src + IMG_F + lane), (lptr_t)(nring + (T & 1) * 64), 4, 0, 0);
    };
    uint64_t best = KEY_SENTINEL;
    float best_d = __builtin_inff();
    stage(0);
    __syncthreads();
    for (int T = 0; T < P.n_ctiles; ++T) {
        if (T + 1 < P.n_ctiles) stage(T + 1);
        if (active) {
            const float* ap = ((T & 1) ? tile1 : tile0) + lane * 4;
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
            for (int t = 0; t < KQ; ++t) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(ap + t * 256);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], b[4 * t + e], acc, 0, 0, 0);
            }
            fold_tile(acc, nring + (T & 1) * 64, xn, T, P.c, h, best, best_d);
        }
        __syncthreads();
    }
    emit(P, best, qt * 32 + q, active && qt * 32 + q < P.n, lane, wave);
}

// D > 256: the row block no longer fits the register file.  Per K step of WIDE_KC blocks a wavefront reads its row
// fragment once and multiplies it into WIDE_TG accumulators, one per centre tile of the group staged in LDS (the
// structure of knn_wide_kernel); each element is still one k-ordered fma chain over the whole row.
__global__ __launch_bounds__(256, 2) void km_assign_wide_kernel(const AssignParams P) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    constexpr int NW = 4, TG = WIDE_TG, KC = WIDE_KC;
    constexpr int BUF_F = TG * KC * 256;
    float* buf0 = reinterpret_cast<float*>(smem_raw);
    float* buf1 = buf0 + BUF_F;
    float* nring = buf1 + BUF_F;  // [2 groups][TG tiles][64]
    const int kq = P.kq;
    const int64_t TILE_F = tile_stride_floats(kq);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane & 31, h = lane >> 5;
    const int64_t n_qtiles = (P.n + 31) / 32;
    const int64_t qt = (int64_t)blockIdx.x * NW + wave;
    const bool active = qt < n_qtiles;
    const float* qimg = P.xp + (size_t)(active ? qt : 0) * TILE_F;
    const float xn = active ? qimg[(size_t)kq * 256 + q] : 0.f;
    const int spg = kq / KC;
    const int n_groups = (P.n_ctiles + TG - 1) / TG;
    const int total = n_groups * spg;
    auto stage = [&](int step) {
        const int g = step / spg, c = step - g * spg;
        int T = g * TG + wave;
        if (T >= P.n_ctiles) T = P.n_ctiles - 1;  // short last group: a copy of the last tile, never folded
        const float* src = P.cp + (size_t)T * TILE_F;
        float* dst = ((step & 1) ? buf1 : buf0) + wave * KC * 256;
#pragma unroll
        for (int u = 0; u < KC; ++u)
            __builtin_amdgcn_global_load_lds((gptr_t)(src + (size_t)(c * KC + u) * 256 + lane * 4), (lptr_t)(dst + u * 256), 16, 0, 0);
        if (c == 0)
            __builtin_amdgcn_global_load_lds((gptr_t)(src + (size_t)kq * 256 + lane), (lptr_t)(nring + ((g & 1) * TG + wave) * 64), 4, 0, 0);
    };
    f32x4 bcur[KC], bnext[KC];
    auto load_b = [&](int c, f32x4 (&bb)[KC]) {
#pragma unroll
        for (int u = 0; u < KC; ++u) bb[u] = *reinterpret_cast<const f32x4*>(qimg + (size_t)(c * KC + u) * 256 + lane * 4);
    };
    uint64_t best = KEY_SENTINEL;
    float best_d = __builtin_inff();
    if (total > 0) { stage(0); load_b(0, bcur); }
    __syncthreads();
    f32x16 acc[TG];
    int g = 0, c = 0;
    for (int step = 0; step < total; ++step) {
        if (step + 1 < total) {
            stage(step + 1);
            load_b((c + 1 == spg) ? 0 : c + 1, bnext);
        }
        if (c == 0) {
#pragma unroll
            for (int j = 0; j < TG; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
        }
        const float* ap = ((step & 1) ? buf1 : buf0) + lane * 4;
#pragma unroll
        for (int j = 0; j < TG; ++j) {
            f32x4 a[KC];
#pragma unroll
            for (int u = 0; u < KC; ++u) a[u] = *reinterpret_cast<const f32x4*>(ap + (j * KC + u) * 256);
#pragma unroll
            for (int u = 0; u < KC; ++u)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][e], bcur[u][e], acc[j], 0, 0, 0);
        }
        if (c == spg - 1) {
            if (active) {
#pragma unroll
                for (int j = 0; j < TG; ++j) {
                    const int T = g * TG + j;
                    if (T < P.n_ctiles) fold_tile(acc[j], nring + ((g & 1) * TG + j) * 64, xn, T, P.c, h, best, best_d);
                }
            }
            c = 0; ++g;
        } else {
            ++c;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < KC; ++u) bcur[u] = bnext[u];
    }
    emit(P, best, qt * 32 + q, active && qt * 32 + q < P.n, lane, wave);
}

// out[0] = sum of the workgroup partials, float64: strided per thread, then a fixed tree
__global__ __launch_bounds__(256) void km_fold_kernel(const double* __restrict__ partial, int64_t m, double* __restrict__ out) {
    __shared__ double red[256];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < m; i += 256) s += partial[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = red[0];
}

// ---- update ------------------------------------------------------------------------------------------------------------

// H[l * nb + row / rpb] += 1 (integer atomics: the counts do not depend on the order)
__global__ __launch_bounds__(256) void km_hist_kernel(const int32_t* __restrict__ labels, int64_t n, int64_t c, int nb, int64_t rpb,
                                                      int32_t* __restrict__ H) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int32_t l = labels[i];
    if (l < 0 || l >= c) return;
    atomicAdd(H + (int64_t)l * nb + i / rpb, 1);
}

// Exclusive scan of m int32 in place (a has m + 1 entries; a[m] = total).  One workgroup: each thread owns a contiguous
// run, sums it, the run sums are scanned in LDS, the runs are rewritten.
__global__ __launch_bounds__(SCAN_THREADS) void km_scan_kernel(int32_t* __restrict__ a, int64_t m) {
    __shared__ int32_t part[SCAN_THREADS];
    const int t = threadIdx.x;
    const int64_t per = (m + SCAN_THREADS - 1) / SCAN_THREADS;
    const int64_t i0 = t * per;
    const int64_t i1 = (i0 + per < m) ? i0 + per : m;
    int32_t s = 0;
    for (int64_t i = i0; i < i1; ++i) s += a[i];
    part[t] = s;
    __syncthreads();
    for (int o = 1; o < SCAN_THREADS; o <<= 1) {  // Hillis-Steele inclusive scan of the run sums
        const int32_t v = (t >= o) ? part[t - o] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int32_t run = part[t] - s;
    for (int64_t i = i0; i < i1; ++i) {
        const int32_t v = a[i];
        a[i] = run;
        run += v;
    }
    if (t == SCAN_THREADS - 1) a[m] = part[t];
}

// From the scanned H: starts (c + 1), counts (c), segments of every cluster (segall) and of the multi-segment ones
// (segmulti, 0 for a cluster of at most SEG rows); both segment arrays have c + 1 entries for their scans.
__global__ __launch_bounds__(256) void km_counts_kernel(const int32_t* __restrict__ Hs, int64_t c, int nb, int32_t* __restrict__ starts,
                                                        int32_t* __restrict__ counts, int32_t* __restrict__ segall,
                                                        int32_t* __restrict__ segmulti) {
    const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (l > c) return;
    if (l == c) { starts[c] = Hs[c * nb]; return; }
    const int32_t s0 = Hs[l * nb], cnt = Hs[(l + 1) * nb] - s0;
    const int32_t ns = (cnt + SEG - 1) / SEG;
    starts[l] = s0;
    counts[l] = cnt;
    segall[l] = ns;
    segmulti[l] = ns > 1 ? ns : 0;
}

// Stable scatter: block b walks its rows in order, 256 at a time; a row's place is its block's cursor for its label plus
// the number of earlier rows of the batch with that label.  Cursors are the scanned H, advanced in place.
__global__ __launch_bounds__(256) void km_scatter_kernel(const int32_t* __restrict__ labels, int64_t n, int64_t c, int nb, int64_t rpb,
                                                         int32_t* __restrict__ H, int32_t* __restrict__ perm) {
    __shared__ int32_t lab[256];
    const int b = blockIdx.x, t = threadIdx.x;
    const int64_t r0 = (int64_t)b * rpb;
    const int64_t r1 = (r0 + rpb < n) ? r0 + rpb : n;
    for (int64_t base = r0; base < r1; base += 256) {
        const int64_t row = base + t;
        int32_t l = -1;
        if (row < r1) {
            l = labels[row];
            if (l < 0 || l >= c) l = -1;
        }
        lab[t] = l;
        __syncthreads();
        int rank = 0;
        bool last = true;
        for (int u = 0; u < 256; ++u) {
            const int32_t lu = lab[u];
            if (u < t) rank += (lu == l) ? 1 : 0;
            else if (u > t && lu == l) last = false;
        }
        int32_t pos = 0;
        if (l >= 0) pos = H[(int64_t)l * nb + b] + rank;
        __syncthreads();
        if (l >= 0) {
            perm[pos] = (int32_t)row;
            if (last) H[(int64_t)l * nb + b] = pos + 1;
        }
        __syncthreads();
    }
}

// One (segment, 64-column block): the float64 sum over the segment's rows in sorted (= ascending row) order.
__global__ __launch_bounds__(64) void km_segsum_kernel(const float* __restrict__ X, int d, int64_t ldx, int64_t c,
                                                       const int32_t* __restrict__ perm, const int32_t* __restrict__ starts,
                                                       const int32_t* __restrict__ segoff, const int32_t* __restrict__ multoff,
                                                       double* __restrict__ partial, float* __restrict__ centres) {
    const int64_t gs = blockIdx.x;
    if (gs >= segoff[c]) return;
    int64_t lo = 0, hi = c;  // largest l with segoff[l] <= gs (segoff is non-decreasing, segoff[c] > gs)
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (segoff[mid] <= gs) lo = mid; else hi = mid;
    }
    while (segoff[lo + 1] <= gs) ++lo;  // skip empty clusters that share the offset
    const int64_t l = lo;
    const int64_t s = gs - segoff[l];
    const int64_t p0 = starts[l] + s * SEG;
    const int64_t pe = starts[l + 1];
    const int64_t p1 = (p0 + SEG < pe) ? p0 + SEG : pe;
    const int col = blockIdx.y * 64 + threadIdx.x;
    if (col >= d) return;
    double acc = 0.0;
    for (int64_t p = p0; p < p1; ++p) acc += (double)X[(int64_t)perm[p] * ldx + col];
    const int64_t cnt = pe - starts[l];
    if (cnt <= SEG) centres[l * d + col] = (float)(acc / (double)cnt);
    else partial[(int64_t)(multoff[l] + s) * d + col] = acc;
}

// Clusters of more than one segment: fold the segment partials in order, mean rounded to fp32 once.
__global__ __launch_bounds__(64) void km_finalize_kernel(int d, int64_t c, const int32_t* __restrict__ starts,
                                                         const int32_t* __restrict__ multoff, const double* __restrict__ partial,
                                                         float* __restrict__ centres) {
    const int64_t l = blockIdx.x;
    const int64_t cnt = starts[l + 1] - starts[l];
    if (cnt <= SEG) return;
    const int col = blockIdx.y * 64 + threadIdx.x;
    if (col >= d) return;
    const int64_t ns = (cnt + SEG - 1) / SEG;
    double acc = 0.0;
    for (int64_t s = 0; s < ns; ++s) acc += partial[(int64_t)(multoff[l] + s) * d + col];
    centres[l * d + col] = (float)(acc / (double)cnt);
}

// ---- empty clusters ----------------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// faiss split_clusters: for every empty centre ci in ascending order, draw a host cluster cj with probability
// (size - 1) / sum(size - 1) (u = splitmix64(seed ^ splitmix64(iter << 32 | ci)) mod that sum, the first cj whose running
// sum exceeds u), copy its centre and push the pair apart by -/+ 1/1024 per coordinate (even coordinates: ci * (1 + eps),
// cj * (1 - eps); odd: the other way), then split the size evenly.  No host (every size <= 1): ci is left as it is.
__global__ __launch_bounds__(256) void km_split_kernel(float* __restrict__ centres, int64_t c, int d, int32_t* __restrict__ counts,
                                                       uint64_t seed, int iter) {
    __shared__ int any_empty;
    __shared__ int64_t pick;
    const int t = threadIdx.x;
    if (t == 0) any_empty = 0;
    __syncthreads();
    for (int64_t l = t; l < c; l += 256)
        if (counts[l] == 0) any_empty = 1;
    __syncthreads();
    if (!any_empty) return;
    const float up = 1.0f + 1.0f / 1024.0f, down = 1.0f - 1.0f / 1024.0f;
    for (int64_t ci = 0; ci < c; ++ci) {
        if (t == 0) {
            pick = -1;
            if (counts[ci] == 0) {
                int64_t total = 0;
                for (int64_t j = 0; j < c; ++j) total += counts[j] > 1 ? counts[j] - 1 : 0;
                if (total > 0) {
                    const uint64_t u = splitmix64(seed ^ splitmix64(((uint64_t)(uint32_t)iter << 32) | (uint64_t)(uint32_t)ci)) %
                                       (uint64_t)total;
                    int64_t run = 0;
                    for (int64_t j = 0; j < c; ++j) {
                        run += counts[j] > 1 ? counts[j] - 1 : 0;
                        if ((uint64_t)run > u) { pick = j; break; }
                    }
                }
            }
        }
        __syncthreads();
        const int64_t cj = pick;
        if (cj >= 0) {
            for (int k = t; k < d; k += 256) {
                const float v = centres[cj * d + k];
                if ((k & 1) == 0) { centres[ci * d + k] = v * up; centres[cj * d + k] = v * down; }
                else { centres[ci * d + k] = v * down; centres[cj * d + k] = v * up; }
            }
            if (t == 0) {
                const int32_t half = counts[cj] / 2;
                counts[ci] = half;
                counts[cj] -= half;
            }
        }
        __syncthreads();
    }
}

static inline int pick_kq(int d) {
    if (d <= 32) return 4;
    if (d <= 64) return 8;
    if (d <= 128) return 16;
    if (d <= 256) return 32;
    return 0;
}
static inline int wide_kq(int d) { return d > 256 ? ((d + 31) / 32) * 4 : 0; }

static inline int nblocks(int64_t n, int64_t c) {
    int64_t nb = HIST_BUDGET / c;
    const int64_t max_nb = (n + 255) / 256;
    if (nb > max_nb) nb = max_nb;
    if (nb < 1) nb = 1;
    return (int)nb;
}

struct UpdateWs {  // byte offsets into the update workspace
    int64_t H, starts, segall, segmulti, partial, total;
};
static UpdateWs update_layout(int64_t n, int64_t c, int d) {
    const int nb = nblocks(n, c);
    auto up = [](int64_t b) { return (b + 255) / 256 * 256; };
    UpdateWs w;
    w.H = 0;
    w.starts = up(w.H + (c * nb + 1) * 4);
    w.segall = up(w.starts + (c + 1) * 4);
    w.segmulti = up(w.segall + (c + 1) * 4);
    w.partial = up(w.segmulti + (c + 1) * 4);
    const int64_t slots = 2 * ((n + SEG - 1) / SEG);  // segments of clusters longer than SEG rows: < 2 n / SEG
    w.total = w.partial + slots * d * 8;
    return w;
}

}  // namespace km
}  // namespace tdr

using namespace tdr::km;

extern "C" {

int64_t tdr_kmeans_assign_ws_bytes(int64_t n) {
    if (n <= 0) return 0;
    return ((n + 127) / 128) * (int64_t)sizeof(double);
}

int tdr_kmeans_assign_f32(const float* xp, int64_t n, const float* cp, int64_t c, int d, int32_t* labels, float* dist,
                          double* obj, void* ws, int64_t ws_bytes, void* stream) {
    if (!xp || !cp || !labels || !dist || !obj || n <= 0 || c <= 0 || d <= 0) return TDR_ERR_BAD_ARG;
    if (n > 0x7fffffffLL || c > 0x7fffffffLL) return TDR_ERR_UNSUPPORTED;
    const int64_t wgs = (n + 127) / 128;
    if (!ws || ws_bytes < wgs * (int64_t)sizeof(double)) return TDR_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    AssignParams P;
    P.xp = xp; P.n = n; P.cp = cp; P.c = c; P.n_ctiles = (int)((c + TILE_ROWS - 1) / TILE_ROWS);
    P.labels = labels; P.dist = dist; P.partial = (double*)ws;
    if (d <= 256) {
        const int kq = pick_kq(d);
        P.kq = kq;
        const size_t lds = (size_t)2 * kq * 256 * sizeof(float) + 2 * 64 * sizeof(float);
        switch (kq) {
            case 4: hipLaunchKernelGGL(km_assign_kernel<4>, dim3((unsigned)wgs), dim3(256), lds, st, P); break;
            case 8: hipLaunchKernelGGL(km_assign_kernel<8>, dim3((unsigned)wgs), dim3(256), lds, st, P); break;
            case 16: hipLaunchKernelGGL(km_assign_kernel<16>, dim3((unsigned)wgs), dim3(256), lds, st, P); break;
            default: {
                hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(km_assign_kernel<32>),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
                if (e != hipSuccess) return (int)e;
                hipLaunchKernelGGL(km_assign_kernel<32>, dim3((unsigned)wgs), dim3(256), lds, st, P);
            }
        }
    } else {
        P.kq = wide_kq(d);
        const size_t lds = (size_t)2 * WIDE_TG * WIDE_KC * 256 * sizeof(float) + (size_t)2 * WIDE_TG * 64 * sizeof(float);
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(km_assign_wide_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(km_assign_wide_kernel, dim3((unsigned)wgs), dim3(256), lds, st, P);
    }
    TDR_CHECK_LAUNCH();
    hipLaunchKernelGGL(km_fold_kernel, dim3(1), dim3(256), 0, st, (const double*)ws, wgs, obj);
    TDR_CHECK_LAUNCH();
    return TDR_OK;
}

int64_t tdr_kmeans_update_ws_bytes(int64_t n, int64_t c, int d) {
    if (n <= 0 || c <= 0 || c > n || d <= 0) return 0;
    return update_layout(n, c, d).total;
}

int tdr_kmeans_update_f32(const float* X, int64_t n, int d, int64_t ldx, const int32_t* labels, int64_t c, float* centres,
                          int32_t* counts, int32_t* perm, void* ws, int64_t ws_bytes, void* stream) {
    if (!X || !labels || !centres || !counts || !perm || n <= 0 || d <= 0 || ldx < d || c <= 0 || c > n) return TDR_ERR_BAD_ARG;
    if (n > 0x7fffffffLL) return TDR_ERR_UNSUPPORTED;
    const UpdateWs w = update_layout(n, c, d);
    if (!ws || ws_bytes < w.total) return TDR_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)ws;
    int32_t* H = (int32_t*)(base + w.H);
    int32_t* starts = (int32_t*)(base + w.starts);
    int32_t* segall = (int32_t*)(base + w.segall);
    int32_t* segmulti = (int32_t*)(base + w.segmulti);
    double* partial = (double*)(base + w.partial);
    const int nb = nblocks(n, c);
    const int64_t rpb = (n + nb - 1) / nb;
    const int64_t m = c * nb;
    hipError_t e = hipMemsetAsync(H, 0, (size_t)(m + 1) * 4, st);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(km_hist_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, labels, n, c, nb, rpb, H);
    TDR_CHECK_LAUNCH();
    hipLaunchKernelGGL(km_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, H, m);
    TDR_CHECK_LAUNCH();
    hipLaunchKernelGGL(km_counts_kernel, dim3((unsigned)((c + 1 + 255) / 256)), dim3(256), 0, st, (const int32_t*)H, c, nb, starts,
                       counts, segall, segmulti);
    TDR_CHECK_LAUNCH();
    hipLaunchKernelGGL(km_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, segall, c);
    TDR_CHECK_LAUNCH();
    hipLaunchKernelGGL(km_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, segmulti, c);
    TDR_CHECK_LAUNCH();
    hipLaunchKernelGGL(km_scatter_kernel, dim3((unsigned)nb), dim3(256), 0, st, labels, n, c, nb, rpb, H, perm);
    TDR_CHECK_LAUNCH();
    const int64_t seg_bound = (n + SEG - 1) / SEG + c;  // >= segall[c]
    const unsigned colb = (unsigned)((d + 63) / 64);
    hipLaunchKernelGGL(km_segsum_kernel, dim3((unsigned)seg_bound, colb), dim3(64), 0, st, X, d, ldx, c, (const int32_t*)perm,
                       (const int32_t*)starts, (const int32_t*)segall, (const int32_t*)segmulti, partial, centres);
    TDR_CHECK_LAUNCH();
    hipLaunchKernelGGL(km_finalize_kernel, dim3((unsigned)c, colb), dim3(64), 0, st, d, c, (const int32_t*)starts,
                       (const int32_t*)segmulti, (const double*)partial, centres);
    TDR_CHECK_LAUNCH();
    return TDR_OK;
}

int tdr_kmeans_split_f32(float* centres, int64_t c, int d, int32_t* counts, uint64_t seed, int iter, void* stream) {
    if (!centres || !counts || c <= 0 || d <= 0) return TDR_ERR_BAD_ARG;
    hipLaunchKernelGGL(km_split_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, centres, c, d, counts, seed, iter);
    TDR_CHECK_LAUNCH();
    return TDR_OK;
}

}  // extern "C"
