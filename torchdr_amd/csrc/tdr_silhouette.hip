// Exact, matrix-free silhouette coefficients (eval/silhouette.py:21-163 of the reference).
//
// The reference loops over pairs of labels in Python and materialises every n_i x n_j block of distances.  Here nothing of
// size N^2 or N*L exists.  The columns are permuted by label (a stable sort on the host), so that every label is one
// contiguous run of columns; a lane owns one row i and streams the columns, keeping only
//   - the running (compensated) weighted distance sum of the current run,
//   - the sum over its own label,
//   - the running minimum over the completed runs of other labels of sum / W_l.
// All lanes of a wavefront see the same column at the same time, so the "label changed" branch is uniform.
//
// Columns are split into segments over the grid (blockIdx.y).  A segment leaves, per row, the partial state
//   (first label, first partial sum; min over the runs it saw whole; last label, last partial sum; own-label sum),
// and sil_finish_kernel folds the segments of a row in segment order (no float atomics: bit-identical from run to run).
// A segment with a single run has first label == last label and its whole sum in the first slot.
//
//   a_i = sum_{j in C(i)} w_j d_ij / (W_C(i) - w_i)    (0 for a point alone in its cluster, as the reference)
//   b_i = min_{l != C(i)} sum_{j in l} w_j d_ij / W_l   (+inf for a single label)
//   s_i = nan_to_num((b_i - a_i) / max(a_i, b_i), 0)
#include "tdr_common.h"

namespace tdr {

// per-row partial state of one segment, structure of arrays of n_seg * n entries each
template <typename T>
struct SilPart {
    int32_t* lab_first;
    int32_t* lab_last;
    T* sum_first;
    T* sum_last;
    T* minb;
    T* own;
};

template <typename T>
static SilPart<T> sil_part_layout(void* ws, int64_t cnt) {
    SilPart<T> p;
    char* c = (char*)ws;
    p.sum_first = (T*)c; c += cnt * sizeof(T);
    p.sum_last = (T*)c; c += cnt * sizeof(T);
    p.minb = (T*)c; c += cnt * sizeof(T);
    p.own = (T*)c; c += cnt * sizeof(T);
    p.lab_first = (int32_t*)c; c += cnt * sizeof(int32_t);
    p.lab_last = (int32_t*)c;
    return p;
}

static int64_t sil_ws_bytes(int64_t n, int n_seg, int tbytes) {
    return (int64_t)n_seg * n * (4 * (int64_t)tbytes + 2 * (int64_t)sizeof(int32_t));
}

// the running state of one row over one segment of columns
template <typename T>
struct SilScan {
    int own_lab, cur_lab, first_lab;
    T cur, comp;       // compensated sum of the open run (float); comp stays 0 for double
    T own, minb, first_sum;
    __device__ __forceinline__ void init(int own_label) {
        own_lab = own_label; cur_lab = -1; first_lab = -1;
        cur = T(0); comp = T(0); own = T(0); minb = (T)__builtin_inf(); first_sum = T(0);
    }
    __device__ __forceinline__ void add(T x) {
        if constexpr (sizeof(T) == 4) {
            const T y = x - comp;
            const T t = cur + y;
            comp = (t - cur) - y;
            cur = t;
        } else {
            cur += x;
        }
    }
    // close the open run and open one of label `lab`; the first run of the segment may continue the previous segment's
    // last one, so it is kept apart for the fold
    __device__ __forceinline__ void open(int lab, const T* __restrict__ W) {
        if (cur_lab >= 0) {
            const T s = cur - comp;
            if (first_lab < 0) { first_lab = cur_lab; first_sum = s; }
            else if (cur_lab == own_lab) own = s;
            else minb = fmin(minb, s / W[cur_lab]);
        }
        cur_lab = lab; cur = T(0); comp = T(0);
    }
    __device__ __forceinline__ void save(const SilPart<T>& p, size_t idx) const {
        const T s = cur - comp;
        if (first_lab < 0) {   // one run only
            p.lab_first[idx] = cur_lab; p.sum_first[idx] = s; p.lab_last[idx] = cur_lab; p.sum_last[idx] = T(0);
        } else {
            p.lab_first[idx] = first_lab; p.sum_first[idx] = first_sum; p.lab_last[idx] = cur_lab; p.sum_last[idx] = s;
        }
        p.minb[idx] = minb; p.own[idx] = own;
    }
};

template <int METRIC, typename T>
__device__ __forceinline__ T sil_term(T acc, T diff) {
    if constexpr (METRIC == 0) return fma(diff, diff, acc);
    else return acc + fabs(diff);
}
template <int METRIC, typename T>
__device__ __forceinline__ T sil_dist(T acc) {
    if constexpr (METRIC == 0) {
        if constexpr (sizeof(T) == 4) return __builtin_amdgcn_sqrtf(acc);
        else return sqrt(acc);
    } else {
        return acc;
    }
}

// fold TC distances of one tile (labels sorted) into the scan; a tile of one label (the common case) is summed plainly first
// and enters the compensated sum once
template <int TC, typename T>
__device__ __forceinline__ void sil_fold_tile(SilScan<T>& sc, const T (&dist)[TC], const int* __restrict__ labs,
                                              const T* __restrict__ wts, int nv, const T* __restrict__ W) {
    const int l0 = labs[0];
    if (nv == TC && labs[TC - 1] == l0) {
        if (l0 != sc.cur_lab) sc.open(l0, W);
        T loc = T(0);
#pragma unroll
        for (int c = 0; c < TC; ++c) loc = fma(wts[c], dist[c], loc);
        sc.add(loc);
        return;
    }
#pragma unroll
    for (int c = 0; c < TC; ++c) {
        if (c < nv) {
            const int l = labs[c];
            if (l != sc.cur_lab) sc.open(l, W);
            sc.add(wts[c] * dist[c]);
        }
    }
}

// Small D (DP in {2, 3, 4, 8, 16}, zero-padded on the host): the row's coordinates stay in registers, the column tile
// (TC = 64 columns, dimension-major) in LDS.  XT: (DP, n) row-major, sorted order.
template <typename T, int METRIC, int DP>
__global__ __launch_bounds__(256) void sil_direct_small_kernel(const T* __restrict__ XT, int64_t n, const int32_t* __restrict__ lab,
                                                               const T* __restrict__ w, const T* __restrict__ W, int64_t seg_cols,
                                                               SilPart<T> part) {
    constexpr int TC = 64;
    __shared__ T ys[DP][TC];
    __shared__ T ws_[TC];
    __shared__ int ls[TC];
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * 256 + tid;
    const bool valid = i < n;
    const int64_t c_begin = (int64_t)blockIdx.y * seg_cols;
    const int64_t c_end = (c_begin + seg_cols < n) ? c_begin + seg_cols : n;
    T xi[DP];
#pragma unroll
    for (int k = 0; k < DP; ++k) xi[k] = valid ? XT[(size_t)k * n + i] : T(0);
    SilScan<T> sc;
    sc.init(valid ? lab[i] : -1);
    for (int64_t c0 = c_begin; c0 < c_end; c0 += TC) {
        const int nv = (int)((c_end - c0 < TC) ? c_end - c0 : TC);
        __syncthreads();
        for (int e = tid; e < DP * TC; e += 256) {
            const int k = e / TC, c = e % TC;
            ys[k][c] = (c < nv) ? XT[(size_t)k * n + c0 + c] : T(0);
        }
        if (tid < TC) {
            ws_[tid] = (tid < nv) ? (w ? w[c0 + tid] : T(1)) : T(0);
            ls[tid] = (tid < nv) ? lab[c0 + tid] : -1;
        }
        __syncthreads();
        T dist[TC];
#pragma unroll
        for (int c = 0; c < TC; ++c) {
            T acc = T(0);
#pragma unroll
            for (int k = 0; k < DP; ++k) acc = sil_term<METRIC>(acc, xi[k] - ys[k][c]);
            dist[c] = sil_dist<METRIC>(acc);
        }
        sil_fold_tile<TC>(sc, dist, ls, ws_, nv, W);
    }
    if (valid) sc.save(part, (size_t)blockIdx.y * n + i);
}

// Any D (padded on the host to a multiple of 16): the column tile (TC = 32 columns) is staged in chunks of KC dimensions,
// the row's coordinates are read 16 at a time from the transposed copy (coalesced over the rows of the workgroup).
template <typename T, int METRIC>
__global__ __launch_bounds__(256) void sil_direct_wide_kernel(const T* __restrict__ XT, int64_t n, int dp, const int32_t* __restrict__ lab,
                                                              const T* __restrict__ w, const T* __restrict__ W, int64_t seg_cols,
                                                              SilPart<T> part) {
    constexpr int TC = 32, KC = 64;
    __shared__ T ys[KC][TC];
    __shared__ T ws_[TC];
    __shared__ int ls[TC];
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * 256 + tid;
    const bool valid = i < n;
    const int64_t c_begin = (int64_t)blockIdx.y * seg_cols;
    const int64_t c_end = (c_begin + seg_cols < n) ? c_begin + seg_cols : n;
    const int64_t ir = valid ? i : 0;
    SilScan<T> sc;
    sc.init(valid ? lab[i] : -1);
    for (int64_t c0 = c_begin; c0 < c_end; c0 += TC) {
        const int nv = (int)((c_end - c0 < TC) ? c_end - c0 : TC);
        T acc[TC];
#pragma unroll
        for (int c = 0; c < TC; ++c) acc[c] = T(0);
        for (int k0 = 0; k0 < dp; k0 += KC) {
            const int kc = (dp - k0 < KC) ? dp - k0 : KC;   // a multiple of 16
            __syncthreads();
            for (int e = tid; e < kc * TC; e += 256) {
                const int k = e / TC, c = e % TC;
                ys[k][c] = (c < nv) ? XT[(size_t)(k0 + k) * n + c0 + c] : T(0);
            }
            if (k0 == 0 && tid < TC) {
                ws_[tid] = (tid < nv) ? (w ? w[c0 + tid] : T(1)) : T(0);
                ls[tid] = (tid < nv) ? lab[c0 + tid] : -1;
            }
            __syncthreads();
            for (int k1 = 0; k1 < kc; k1 += 16) {
                T xi[16];
#pragma unroll
                for (int k = 0; k < 16; ++k) xi[k] = XT[(size_t)(k0 + k1 + k) * n + ir];
#pragma unroll
                for (int k = 0; k < 16; ++k) {
#pragma unroll
                    for (int c = 0; c < TC; ++c) acc[c] = sil_term<METRIC>(acc[c], xi[k] - ys[k1 + k][c]);
                }
            }
        }
        T dist[TC];
#pragma unroll
        for (int c = 0; c < TC; ++c) dist[c] = sil_dist<METRIC>(acc[c]);
        sil_fold_tile<TC>(sc, dist, ls, ws_, nv, W);
    }
    if (valid) sc.save(part, (size_t)blockIdx.y * n + i);
}

// Fold the partial state of the next segment (lf, sf; mb; ll, sl; ow) into a row's running fold (open run, min, own sum).
template <typename T>
__device__ __forceinline__ void sil_fold_state(int& open_lab, T& open_sum, T& minb, T& own, int own_lab, const T* __restrict__ W,
                                               int lf, T sf, T mb, int ll, T sl, T ow) {
    if (lf < 0) return;   // an empty segment
    auto close = [&]() {
        if (open_lab < 0) return;
        if (open_lab == own_lab) own += open_sum;
        else minb = fmin(minb, open_sum / W[open_lab]);
    };
    if (lf == open_lab) {
        open_sum += sf;
    } else {
        close();
        open_lab = lf; open_sum = sf;
    }
    minb = fmin(minb, mb);   // +inf / 0 for a segment of one run
    own += ow;
    if (lf != ll) {
        close();
        open_lab = ll; open_sum = sl;
    }
}

// Precomputed (n, n) distances (row stride ldd, ORIGINAL order): one workgroup per sorted row r; thread t scans the sorted
// columns [t*chunk, (t+1)*chunk) as a segment of its own, and thread 0 folds the 256 states in order into segment 0 of the
// workspace.  The diagonal is read as given (the reference keeps it).
template <typename T>
__global__ __launch_bounds__(256) void sil_precomputed_kernel(const T* __restrict__ Dm, int64_t ldd, int64_t n, const int64_t* __restrict__ perm,
                                                              const int32_t* __restrict__ lab, const T* __restrict__ w,
                                                              const T* __restrict__ W, SilPart<T> part) {
    __shared__ int s_lf[256], s_ll[256];
    __shared__ T s_sf[256], s_sl[256], s_mb[256], s_ow[256];
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x;
    const T* __restrict__ row = Dm + (size_t)perm[r] * ldd;
    const int own_lab = lab[r];
    const int64_t chunk = (n + 255) / 256;
    const int64_t j0 = (int64_t)tid * chunk;
    const int64_t j1 = (j0 + chunk < n) ? j0 + chunk : n;
    SilScan<T> sc;
    sc.init(own_lab);
    for (int64_t j = j0; j < j1; ++j) {
        const int l = lab[j];
        if (l != sc.cur_lab) sc.open(l, W);
        const T d = row[perm[j]];
        sc.add(w ? w[j] * d : d);
    }
    {
        const T s = sc.cur - sc.comp;
        if (sc.cur_lab < 0) { s_lf[tid] = -1; s_ll[tid] = -1; s_sf[tid] = T(0); s_sl[tid] = T(0); }
        else if (sc.first_lab < 0) { s_lf[tid] = sc.cur_lab; s_ll[tid] = sc.cur_lab; s_sf[tid] = s; s_sl[tid] = T(0); }
        else { s_lf[tid] = sc.first_lab; s_ll[tid] = sc.cur_lab; s_sf[tid] = sc.first_sum; s_sl[tid] = s; }
        s_mb[tid] = sc.minb; s_ow[tid] = sc.own;
    }
    __syncthreads();
    if (tid == 0) {
        // fold into one single segment state: (open label, open sum) stays open as the "last" run
        int open_lab = -1;
        T open_sum = T(0), minb = (T)__builtin_inf(), own = T(0);
        for (int t = 0; t < 256; ++t)
            sil_fold_state<T>(open_lab, open_sum, minb, own, own_lab, W, s_lf[t], s_sf[t], s_mb[t], s_ll[t], s_sl[t], s_ow[t]);
        // handed over as one segment whose only partial run is the run still open
        part.lab_first[r] = open_lab; part.sum_first[r] = open_sum;
        part.lab_last[r] = open_lab; part.sum_last[r] = T(0);
        part.minb[r] = minb; part.own[r] = own;
    }
}

// W_l = sum of the weights of label l in sorted order (w == NULL: the count), one thread per label: a fixed order
template <typename T>
__global__ __launch_bounds__(256) void sil_label_weights_kernel(const T* __restrict__ w, const int64_t* __restrict__ starts, int64_t L,
                                                                T* __restrict__ W) {
    const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (l >= L) return;
    const int64_t b = starts[l], e = starts[l + 1];
    if (!w) { W[l] = (T)(e - b); return; }
    double s = 0.0;
    for (int64_t j = b; j < e; ++j) s += (double)w[j];
    W[l] = (T)s;
}

// fold the segments of a sorted row in segment order, form a, b and s, and scatter to the original order
template <typename T>
__global__ __launch_bounds__(256) void sil_finish_kernel(SilPart<T> part, int64_t n, int n_seg, const int32_t* __restrict__ lab,
                                                         const T* __restrict__ w, const T* __restrict__ W,
                                                         const int64_t* __restrict__ starts, const int64_t* __restrict__ perm,
                                                         T* __restrict__ s_out, T* __restrict__ a_out, T* __restrict__ b_out) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const int own_lab = lab[r];
    int open_lab = -1;
    T open_sum = T(0), minb = (T)__builtin_inf(), own = T(0);
    for (int sg = 0; sg < n_seg; ++sg) {
        const size_t idx = (size_t)sg * n + r;
        sil_fold_state<T>(open_lab, open_sum, minb, own, own_lab, W, part.lab_first[idx], part.sum_first[idx], part.minb[idx],
                          part.lab_last[idx], part.sum_last[idx], part.own[idx]);
    }
    if (open_lab >= 0) {
        if (open_lab == own_lab) own += open_sum;
        else minb = fmin(minb, open_sum / W[open_lab]);
    }
    const int64_t n_c = starts[own_lab + 1] - starts[own_lab];
    const T wi = w ? w[r] : T(1);
    const T a = (n_c > 1) ? own / (W[own_lab] - wi) : T(0);
    const T b = minb;
    T s = (b - a) / fmax(a, b);
    if (isnan(s)) s = T(0);
    else if (isinf(s)) s = s > T(0) ? (T)(sizeof(T) == 4 ? 3.40282347e+38 : 1.7976931348623157e+308)
                                    : (T)(sizeof(T) == 4 ? -3.40282347e+38 : -1.7976931348623157e+308);
    const int64_t o = perm[r];
    s_out[o] = s;
    if (a_out) a_out[o] = a;
    if (b_out) b_out[o] = b;
}

// mean of s in float64: 256 threads sum strided slices, then a fixed tree
template <typename T>
__global__ __launch_bounds__(256) void sil_mean_kernel(const T* __restrict__ s, int64_t n, double* __restrict__ out) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (int64_t j = tid; j < n; j += 256) acc += (double)s[j];
    red[tid] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) out[0] = red[0] / (double)n;
}

template <typename T>
static int sil_direct_launch(const T* XT, int64_t n, int dp, const int32_t* lab, const T* w, const T* W, int metric, int n_seg,
                             void* ws, int64_t ws_bytes, hipStream_t st) {
    if (!XT || !lab || !W || !ws || n <= 0 || dp <= 0 || n_seg <= 0 || n_seg > 65535) return TDR_ERR_BAD_ARG;
    if (metric != 0 && metric != 1) return TDR_ERR_BAD_ARG;
    if (n > (int64_t)1 << 31 || ((n + 255) / 256) > 0x7fffffffLL) return TDR_ERR_UNSUPPORTED;
    if (!(dp == 2 || dp == 3 || dp == 4 || dp == 8 || dp == 16 || dp % 16 == 0)) return TDR_ERR_UNSUPPORTED;
    if (ws_bytes < sil_ws_bytes(n, n_seg, (int)sizeof(T))) return TDR_ERR_WORKSPACE;
    // segments of whole 64-column tiles, none empty
    const int64_t seg_cols = ((n + n_seg - 1) / n_seg + 63) / 64 * 64;
    if ((n + seg_cols - 1) / seg_cols != n_seg) return TDR_ERR_BAD_ARG;
    SilPart<T> part = sil_part_layout<T>(ws, (int64_t)n_seg * n);
    const dim3 grid((unsigned)((n + 255) / 256), (unsigned)n_seg);
#define TDR_SIL_SMALL(M, D) hipLaunchKernelGGL((sil_direct_small_kernel<T, M, D>), grid, dim3(256), 0, st, XT, n, lab, w, W, seg_cols, part)
#define TDR_SIL_CASES(M)                           \
    switch (dp) {                                  \
        case 2: TDR_SIL_SMALL(M, 2); break;        \
        case 3: TDR_SIL_SMALL(M, 3); break;        \
        case 4: TDR_SIL_SMALL(M, 4); break;        \
        case 8: TDR_SIL_SMALL(M, 8); break;        \
        case 16: TDR_SIL_SMALL(M, 16); break;      \
        default: hipLaunchKernelGGL((sil_direct_wide_kernel<T, M>), grid, dim3(256), 0, st, XT, n, dp, lab, w, W, seg_cols, part); \
    }
    if (metric == 0) { TDR_SIL_CASES(0) } else { TDR_SIL_CASES(1) }
#undef TDR_SIL_CASES
#undef TDR_SIL_SMALL
    TDR_CHECK_LAUNCH();
    return TDR_OK;
}

template <typename T>
static int sil_precomputed_launch(const T* Dm, int64_t ldd, int64_t n, const int64_t* perm, const int32_t* lab, const T* w,
                                  const T* W, void* ws, int64_t ws_bytes, hipStream_t st) {
    if (!Dm || !perm || !lab || !W || !ws || n <= 0 || ldd < n) return TDR_ERR_BAD_ARG;
    if (n > 0x7fffffffLL) return TDR_ERR_UNSUPPORTED;
    if (ws_bytes < sil_ws_bytes(n, 1, (int)sizeof(T))) return TDR_ERR_WORKSPACE;
    SilPart<T> part = sil_part_layout<T>(ws, n);
    hipLaunchKernelGGL((sil_precomputed_kernel<T>), dim3((unsigned)n), dim3(256), 0, st, Dm, ldd, n, perm, lab, w, W, part);
    TDR_CHECK_LAUNCH();
    return TDR_OK;
}

template <typename T>
static int sil_label_weights_launch(const T* w, const int64_t* starts, int64_t L, T* W, hipStream_t st) {
    if (!starts || !W || L <= 0) return TDR_ERR_BAD_ARG;
    hipLaunchKernelGGL((sil_label_weights_kernel<T>), dim3((unsigned)((L + 255) / 256)), dim3(256), 0, st, w, starts, L, W);
    TDR_CHECK_LAUNCH();
    return TDR_OK;
}

template <typename T>
static int sil_finish_launch(const void* ws, int64_t ws_bytes, int64_t n, int n_seg, const int32_t* lab, const T* w, const T* W,
                             const int64_t* starts, const int64_t* perm, T* s, T* a, T* b, hipStream_t st) {
    if (!ws || !lab || !W || !starts || !perm || !s || n <= 0 || n_seg <= 0) return TDR_ERR_BAD_ARG;
    if (ws_bytes < sil_ws_bytes(n, n_seg, (int)sizeof(T))) return TDR_ERR_WORKSPACE;
    SilPart<T> part = sil_part_layout<T>(const_cast<void*>(ws), (int64_t)n_seg * n);
    hipLaunchKernelGGL((sil_finish_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, part, n, n_seg, lab, w, W, starts,
                       perm, s, a, b);
    TDR_CHECK_LAUNCH();
    return TDR_OK;
}

template <typename T>
static int sil_mean_launch(const T* s, int64_t n, double* out, hipStream_t st) {
    if (!s || !out || n <= 0) return TDR_ERR_BAD_ARG;
    hipLaunchKernelGGL((sil_mean_kernel<T>), dim3(1), dim3(256), 0, st, s, n, out);
    TDR_CHECK_LAUNCH();
    return TDR_OK;
}

}  // namespace tdr

using namespace tdr;

extern "C" {

int64_t tdr_silhouette_workspace_bytes(int64_t n, int n_seg, int dtype_bytes) {
    if (n <= 0 || n_seg <= 0 || (dtype_bytes != 4 && dtype_bytes != 8)) return 0;
    return sil_ws_bytes(n, n_seg, dtype_bytes);
}

int tdr_silhouette_label_weights_f32(const float* w, const int64_t* starts, int64_t L, float* W, void* stream) {
    return sil_label_weights_launch<float>(w, starts, L, W, (hipStream_t)stream);
}
int tdr_silhouette_label_weights_f64(const double* w, const int64_t* starts, int64_t L, double* W, void* stream) {
    return sil_label_weights_launch<double>(w, starts, L, W, (hipStream_t)stream);
}

int tdr_silhouette_direct_f32(const float* XT, int64_t n, int dp, const int32_t* lab, const float* w, const float* W, int metric,
                              int n_seg, void* ws, int64_t ws_bytes, void* stream) {
    return sil_direct_launch<float>(XT, n, dp, lab, w, W, metric, n_seg, ws, ws_bytes, (hipStream_t)stream);
}
int tdr_silhouette_direct_f64(const double* XT, int64_t n, int dp, const int32_t* lab, const double* w, const double* W, int metric,
                              int n_seg, void* ws, int64_t ws_bytes, void* stream) {
    return sil_direct_launch<double>(XT, n, dp, lab, w, W, metric, n_seg, ws, ws_bytes, (hipStream_t)stream);
}

int tdr_silhouette_precomputed_f32(const float* Dm, int64_t ldd, int64_t n, const int64_t* perm, const int32_t* lab, const float* w,
                                   const float* W, void* ws, int64_t ws_bytes, void* stream) {
    return sil_precomputed_launch<float>(Dm, ldd, n, perm, lab, w, W, ws, ws_bytes, (hipStream_t)stream);
}
int tdr_silhouette_precomputed_f64(const double* Dm, int64_t ldd, int64_t n, const int64_t* perm, const int32_t* lab, const double* w,
                                   const double* W, void* ws, int64_t ws_bytes, void* stream) {
    return sil_precomputed_launch<double>(Dm, ldd, n, perm, lab, w, W, ws, ws_bytes, (hipStream_t)stream);
}

int tdr_silhouette_finish_f32(const void* ws, int64_t ws_bytes, int64_t n, int n_seg, const int32_t* lab, const float* w,
                              const float* W, const int64_t* starts, const int64_t* perm, float* s, float* a, float* b, void* stream) {
    return sil_finish_launch<float>(ws, ws_bytes, n, n_seg, lab, w, W, starts, perm, s, a, b, (hipStream_t)stream);
}
int tdr_silhouette_finish_f64(const void* ws, int64_t ws_bytes, int64_t n, int n_seg, const int32_t* lab, const double* w,
                              const double* W, const int64_t* starts, const int64_t* perm, double* s, double* a, double* b,
                              void* stream) {
    return sil_finish_launch<double>(ws, ws_bytes, n, n_seg, lab, w, W, starts, perm, s, a, b, (hipStream_t)stream);
}

int tdr_silhouette_mean_f32(const float* s, int64_t n, double* out, void* stream) {
    return sil_mean_launch<float>(s, n, out, (hipStream_t)stream);
}
int tdr_silhouette_mean_f64(const double* s, int64_t n, double* out, void* stream) {
    return sil_mean_launch<double>(s, n, out, (hipStream_t)stream);
}

}  // extern "C"
