// fs_mapsweep.hip -- the listwise term of fs_maplist.hip as a FUNCTION OF THE PREDICTION TEMPERATURE: for every image with many
// labels and every one of up to 64 temperatures the KL divergence D_b(beta), beta = 1 / T_p, its first and second derivative in
// beta, and what a Boltzmann policy at that temperature earns on the image's recorded cells -- in one pass over the labels
// (flingbot_amd/trainops.py map_list_sweep and fit_temperature; include/flingsim.h has the rule in full).
//
//   fs_k_map_sweep_image   one workgroup per image.  Thread t holds labels t, t + 256, ... of the image -- at most 16 -- in
//                          registers; a slot the image does not reach costs one uniform branch in the passes that run once.
//                          Once per image: the arg-max of p and of y as (value, index) pairs, the sum of exp of the labels
//                          below the maximum, and one block reduction that carries  sum q lq,  sum q d,  sum q  and the
//                          non-finite mark together.  Then the labels become doubles d = p - max p and u = y - max y, a
//                          position the image does not have a sentinel whose exp is 0, and the loop over the temperatures
//                          runs on them without a branch, in the form for 1, 2, 4, 8 or 16 slots that holds the image:
//                          e = exp(beta d) and ONE block reduction of four sums (e without the arg-max's own 1, e d, e d^2, e u);
//                          the two picked values of s need no reduction of their own, since s at the arg-max of p is 1 / sum e
//                          and s at the arg-max of y is exp(beta d_best) / sum e with d_best found once.  The reduction's LDS
//                          slots alternate between two sets, so a temperature costs one barrier.  (No branch may surround a
//                          write to the register arrays: with one, the compiler copies the whole arrays at every merge -- 452
//                          registers, 224 of them accumulation registers as spill space, against 255 and none.)
//   fs_k_map_sweep_finish  one workgroup per temperature: G_l, L_l and the six sums over the images by fs_k_map_list_finish's
//                          schedule (image b on thread b mod 256 in double, 64-lane shuffle, the 4 wave results front to back).
// No atomics, no arrival counters, nothing read back: equal inputs give equal bits, and an image's rows depend on neither its
// place in the batch nor on the other images.  The arg-max order -- larger value first, then lower index, NaN below everything
// -- is total, so the winner does not depend on the shape of the reduction tree.
//
// D_b(beta) = sum_i q_i (lq_i - ls_i) with ls_i = beta d_i - log1p(Z'), Z' the sum of e without the arg-max's own addend, is
// sum q lq - beta sum q d + (sum q) log1p(Z'): the first three sums do not depend on beta.  sum q is 1 up to rounding; keeping it
// keeps D_b the sum fs_map_list_loss forms.  Every moment is taken about max p (and E_s[y] about max y): at a low temperature s
// sits on the arg-max, where d = 0, so Var_s[p] = E_s[d^2] - E_s[d]^2 is a difference of two small numbers, not of two large ones.
//
// Cost on an MI355X (scripts/map_sweep_timing.py, EXPERIMENTS R32.1), 33 / 64 temperatures: 0.047 / 0.081 ms at 32 x 144 labels,
// 0.111 / 0.196 ms at 1000 x 144, 0.088 / 0.150 ms at 1 x 4096, where one fs_map_list_loss call per temperature takes 0.62 / 1.23,
// 0.62 / 1.26 and 0.73 / 1.42 ms.
//
// Offsets are clamped wherever they are read (fs_ms_image, fs_ll_image's rule): begin into [0, L], end into [begin, L] and to
// begin + 4096.  Every index below is formed from the clamped values: a malformed table gives wrong numbers, never an access
// outside the buffers.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>

#include "../../include/flingsim.h"
#include "fs_context.h"

#define FS_MS_THREADS 256
#define FS_MS_WAVES (FS_MS_THREADS / 64)
#define FS_MS_MAX_IMAGE 4096                             // labels of one image
#define FS_MS_SLOTS (FS_MS_MAX_IMAGE / FS_MS_THREADS)    // 16 labels per thread at the most
#define FS_MS_MAX_TEMPERATURES 64

// the reciprocal temperatures, as kernel arguments
struct fs_ms_betas {
    double beta[FS_MS_MAX_TEMPERATURES];
};

struct fs_ms_top {
    float v;
    int k;
};

struct fs_ms_four {
    double a, b, c, d;
};

// [begin, begin + count) of image b, clamped
__device__ __forceinline__ void fs_ms_image(const int *__restrict__ d_offsets, int b, int labels, int &begin, int &count) {
    begin = min(max(d_offsets[b], 0), labels);
    int end = min(max(d_offsets[b + 1], begin), labels);
    end = min(end, begin + FS_MS_MAX_IMAGE);
    count = end - begin;
}

// the larger value, among equals the lower index (v is never NaN here: a total order)
__device__ __forceinline__ fs_ms_top fs_ms_better(fs_ms_top a, fs_ms_top b) {
    return (b.v > a.v || (b.v == a.v && b.k < a.k)) ? b : a;
}

__device__ __forceinline__ fs_ms_top fs_ms_block_top(fs_ms_top t, fs_ms_top *slots, int tid) {
    for (int off = 32; off > 0; off >>= 1) {
        fs_ms_top other;
        other.v = __shfl_down(t.v, off, 64);
        other.k = __shfl_down(t.k, off, 64);
        t = fs_ms_better(t, other);
    }
    __syncthreads();  // the readers of the slots' previous use are done
    if ((tid & 63) == 0) slots[tid >> 6] = t;
    __syncthreads();
    fs_ms_top best = slots[0];
#pragma unroll
    for (int w = 1; w < FS_MS_WAVES; ++w) best = fs_ms_better(best, slots[w]);
    return best;
}

template <typename T>
__device__ __forceinline__ T fs_ms_block_sum(T v, T *slots, int tid) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    __syncthreads();  // the readers of the slots' previous use are done
    if ((tid & 63) == 0) slots[tid >> 6] = v;
    __syncthreads();
    T total = slots[0];
#pragma unroll
    for (int w = 1; w < FS_MS_WAVES; ++w) total += slots[w];
    return total;
}

// four sums in one reduction: 64-lane shuffle, one LDS slot per wave, the 4 slots front to back.  The caller hands in a slot
// set that no thread can still be reading (two sets in turn), so there is ONE barrier.
__device__ __forceinline__ fs_ms_four fs_ms_block_sum4(fs_ms_four v, fs_ms_four *slots, int tid) {
    for (int off = 32; off > 0; off >>= 1) {
        v.a += __shfl_down(v.a, off, 64);
        v.b += __shfl_down(v.b, off, 64);
        v.c += __shfl_down(v.c, off, 64);
        v.d += __shfl_down(v.d, off, 64);
    }
    if ((tid & 63) == 0) slots[tid >> 6] = v;
    __syncthreads();
    fs_ms_four total = slots[0];
#pragma unroll
    for (int w = 1; w < FS_MS_WAVES; ++w) {
        total.a += slots[w].a;
        total.b += slots[w].b;
        total.c += slots[w].c;
        total.d += slots[w].d;
    }
    return total;
}

// a position the image does not have: exp(beta * FS_MS_ABSENT) is exactly 0 for every beta the entry point admits (>= 1e-38), and
// 0 * FS_MS_ABSENT = -0.0, so such a position adds a zero to every sum; a real p - max p is >= -7e38
#define FS_MS_ABSENT (-1.0e300)

// what the loop over the temperatures takes from the pass before it
struct fs_ms_once {
    double q_lq, q_d, q_sum, mark;  // sum q lq,  sum q d,  sum q,  0.0 or NaN
    double max_y, d_best;           // y at its arg-max;  p at the arg-max of y, about max p
};

// The temperatures of one image whose labels reach NS register slots (the caller picks the smallest of 1, 2, 4, 8, 16 that holds
// the image): no branch inside a temperature but the one of the thread that writes.
template <int NS>
__device__ __forceinline__ void fs_ms_sweep(const double (&d)[FS_MS_SLOTS], const double (&u)[FS_MS_SLOTS], int own,
                                            const fs_ms_betas &betas, int n_temperatures, const fs_ms_once &t,
                                            fs_ms_four (*fslots)[FS_MS_WAVES], double *__restrict__ rows,
                                            double *__restrict__ pick, int tid) {
    for (int s = 0; s < n_temperatures; ++s) {
        const double beta = betas.beta[s];
        fs_ms_four acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            const double e = exp(beta * d[k]);  // exactly 1 at the arg-max of p
            const double ed = e * d[k];
            acc.a += k == own ? 0.0 : e;
            acc.b += ed;
            acc.c += ed * d[k];
            acc.d += e * u[k];
        }
        acc = fs_ms_block_sum4(acc, fslots[(s + 1) & 1], tid);
        if (tid == 0) {
            const double z = 1.0 + acc.a;
            const double mean_d = acc.b / z;
            rows[4 * s + 0] = ((t.q_lq - beta * t.q_d) + t.q_sum * log1p(acc.a)) + t.mark;
            rows[4 * s + 1] = (mean_d - t.q_d) + t.mark;
            rows[4 * s + 2] = fmax(acc.c / z - mean_d * mean_d, 0.0) + t.mark;
            rows[4 * s + 3] = (t.max_y + acc.d / z) + t.mark;
            pick[2 * s + 0] = exp(beta * t.d_best) / z + t.mark;  // s at the arg-max of y
            pick[2 * s + 1] = 1.0 / z + t.mark;                   // s at the arg-max of p
        }
    }
}

__global__ __launch_bounds__(FS_MS_THREADS) void fs_k_map_sweep_image(const float *__restrict__ d_pred,
                                                                       const float *__restrict__ d_label,
                                                                       const int *__restrict__ d_offsets, int labels,
                                                                       fs_ms_betas betas, int n_temperatures,
                                                                       double label_temperature, double *__restrict__ d_rows,
                                                                       double *__restrict__ d_images,
                                                                       double *__restrict__ d_picked) {
    __shared__ fs_ms_top tslots[FS_MS_WAVES];
    __shared__ double dslots[FS_MS_WAVES];
    __shared__ fs_ms_four fslots[2][FS_MS_WAVES];
    __shared__ double picked[2];  // y at the arg-max of p, p at the arg-max of y
    const int tid = threadIdx.x, b = blockIdx.x;
    int begin, count;
    fs_ms_image(d_offsets, b, labels, begin, count);
    double *rows = d_rows + (size_t)b * n_temperatures * 4;
    double *pick = d_picked + (size_t)b * n_temperatures * 2;
    if (count < 2) {  // (uniform) not listed: zeros
        for (int k = tid; k < 4 * n_temperatures; k += FS_MS_THREADS) rows[k] = 0.0;
        for (int k = tid; k < 2 * n_temperatures; k += FS_MS_THREADS) pick[k] = 0.0;
        if (tid < 4) d_images[4 * (size_t)b + tid] = 0.0;
        return;
    }

    float pf[FS_MS_SLOTS], yf[FS_MS_SLOTS];  // p and y as loaded
    fs_ms_top top_p = {-INFINITY, INT_MAX}, top_y = {-INFINITY, INT_MAX};
#pragma unroll
    for (int k = 0; k < FS_MS_SLOTS; ++k) {
        pf[k] = 0.0f;
        yf[k] = 0.0f;
        if (k * FS_MS_THREADS < count) {  // (uniform)
            const int i = k * FS_MS_THREADS + tid;
            if (i < count) {
                const float p = d_pred[begin + i], y = d_label[begin + i];
                pf[k] = p;
                yf[k] = y;
                const fs_ms_top cand_p = {p != p ? -INFINITY : p, i}, cand_y = {y != y ? -INFINITY : y, i};  // NaN never wins
                top_p = fs_ms_better(top_p, cand_p);
                top_y = fs_ms_better(top_y, cand_y);
            }
        }
    }
    top_p = fs_ms_block_top(top_p, tslots, tid);  // index 0 exists, so .k lies in [0, count)
    top_y = fs_ms_block_top(top_y, tslots, tid);
    const double max_p = (double)top_p.v, max_y = (double)top_y.v;
    const double max_c = max_y / label_temperature;

    // what does not depend on the temperature: q, and with it  sum q lq,  sum q d,  sum q;  the mark is 0.0 for an image of finite
    // values and NaN otherwise (x - x), and is added to every row entry
    double zc = 0.0;  // the sum of exp without the maximum's own 1
#pragma unroll
    for (int k = 0; k < FS_MS_SLOTS; ++k) {
        if (k * FS_MS_THREADS < count) {
            const int i = k * FS_MS_THREADS + tid;
            if (i < count && i != top_y.k) zc += exp((double)yf[k] / label_temperature - max_c);
        }
    }
    const double log_zc = log1p(fs_ms_block_sum(zc, dslots, tid));
    fs_ms_four once = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < FS_MS_SLOTS; ++k) {
        if (k * FS_MS_THREADS < count) {
            const int i = k * FS_MS_THREADS + tid;
            if (i < count) {
                const double p = (double)pf[k], y = (double)yf[k];
                const double lq = (y / label_temperature - max_c) - log_zc;
                const double q = exp(lq);
                if (i == top_p.k) picked[0] = y;  // (one thread each; read after the barrier of the sum below)
                if (i == top_y.k) picked[1] = p;
                if (q != 0.0) {  // an underflowed q contributes exactly 0
                    once.a += q * lq;
                    once.b += q * (p - max_p);
                    once.c += q;
                }
                once.d += (p - p) + (y - y);
            }
        }
    }
    once = fs_ms_block_sum4(once, fslots[0], tid);
    double d[FS_MS_SLOTS], u[FS_MS_SLOTS];  // p - max p and y - max y; no branch around these, and none in the loops below
#pragma unroll
    for (int k = 0; k < FS_MS_SLOTS; ++k) {
        const bool have = k * FS_MS_THREADS + tid < count;
        d[k] = have ? (double)pf[k] - max_p : FS_MS_ABSENT;
        u[k] = have ? (double)yf[k] - max_y : 0.0;
    }
    if (tid == 0) {
        d_images[4 * (size_t)b + 0] = (double)count;
        d_images[4 * (size_t)b + 1] = max_y;
        d_images[4 * (size_t)b + 2] = picked[0];
        d_images[4 * (size_t)b + 3] = max_p + once.b;  // E_q[p]
    }

    const fs_ms_once terms = {once.a, once.b, once.c, once.d, max_y, picked[1] - max_p};
    const int own = (top_p.k % FS_MS_THREADS) == tid ? top_p.k / FS_MS_THREADS : -1;  // the slot that holds the arg-max of p
    const int reached = (count + FS_MS_THREADS - 1) / FS_MS_THREADS;                  // (uniform)
    if (reached <= 1)
        fs_ms_sweep<1>(d, u, own, betas, n_temperatures, terms, fslots, rows, pick, tid);
    else if (reached <= 2)
        fs_ms_sweep<2>(d, u, own, betas, n_temperatures, terms, fslots, rows, pick, tid);
    else if (reached <= 4)
        fs_ms_sweep<4>(d, u, own, betas, n_temperatures, terms, fslots, rows, pick, tid);
    else if (reached <= 8)
        fs_ms_sweep<8>(d, u, own, betas, n_temperatures, terms, fslots, rows, pick, tid);
    else
        fs_ms_sweep<16>(d, u, own, betas, n_temperatures, terms, fslots, rows, pick, tid);
}

__global__ __launch_bounds__(FS_MS_THREADS) void fs_k_map_sweep_finish(const int *__restrict__ d_offsets, int images, int labels,
                                                                        int n_temperatures, int per_image,
                                                                        const double *__restrict__ d_rows,
                                                                        const double *__restrict__ d_images,
                                                                        const double *__restrict__ d_picked,
                                                                        double *__restrict__ d_curve) {
    __shared__ double dslots[FS_MS_WAVES];
    __shared__ long long lslots[FS_MS_WAVES];
    const int tid = threadIdx.x, s = blockIdx.x;
    double kl_acc = 0.0, slope_acc = 0.0, curv_acc = 0.0, regret_acc = 0.0, best_acc = 0.0, greedy_acc = 0.0;
    long long listed_acc = 0, labels_acc = 0;
    for (int b = tid; b < images; b += FS_MS_THREADS) {
        int begin, count;
        fs_ms_image(d_offsets, b, labels, begin, count);
        if (count < 2) continue;
        const double *row = d_rows + ((size_t)b * n_temperatures + s) * 4;
        const double *pick = d_picked + ((size_t)b * n_temperatures + s) * 2;
        const double k = per_image ? 1.0 : (double)count;
        kl_acc += k * row[0];
        slope_acc += k * row[1];
        curv_acc += k * row[2];
        regret_acc += d_images[4 * (size_t)b + 1] - row[3];
        best_acc += pick[0];
        greedy_acc += pick[1];
        listed_acc += 1;
        labels_acc += count;
    }
    const double kl_total = fs_ms_block_sum(kl_acc, dslots, tid);
    const double slope_total = fs_ms_block_sum(slope_acc, dslots, tid);
    const double curv_total = fs_ms_block_sum(curv_acc, dslots, tid);
    const double regret_total = fs_ms_block_sum(regret_acc, dslots, tid);
    const double best_total = fs_ms_block_sum(best_acc, dslots, tid);
    const double greedy_total = fs_ms_block_sum(greedy_acc, dslots, tid);
    const long long listed = fs_ms_block_sum(listed_acc, lslots, tid);         // G_l
    const long long listed_labels = fs_ms_block_sum(labels_acc, lslots, tid);  // L_l
    if (tid == 0) {
        const double norm = (double)(per_image ? listed : listed_labels);
        double *out = d_curve + 8 * (size_t)s;
        out[0] = listed > 0 ? kl_total / norm : 0.0;
        out[1] = listed > 0 ? slope_total / norm : 0.0;
        out[2] = listed > 0 ? curv_total / norm : 0.0;
        out[3] = listed > 0 ? regret_total / (double)listed : 0.0;
        out[4] = listed > 0 ? best_total / (double)listed : 0.0;
        out[5] = listed > 0 ? greedy_total / (double)listed : 0.0;
        out[6] = (double)listed;
        out[7] = (double)listed_labels;
    }
}

static bool fs_ms_served(int images, int labels, int n_temperatures) {
    return images >= 1 && labels >= 1 && n_temperatures >= 1 && n_temperatures <= FS_MS_MAX_TEMPERATURES;
}

// positive and finite, as a double and as a float
static bool fs_ms_positive(double v) { return std::isfinite(v) && v > 0.0 && std::isfinite((float)v) && (float)v > 0.0f; }

extern "C" size_t fs_map_list_sweep_work_bytes(int images, int labels, int n_temperatures) {
    if (!fs_ms_served(images, labels, n_temperatures)) return 0;
    return (size_t)images * (size_t)n_temperatures * 2 * sizeof(double);  // the two picked s per image and temperature
}

extern "C" int fs_map_list_sweep(const float *d_pred, const float *d_label, const int *d_offsets, int images, int labels,
                                 const double *temperatures, int n_temperatures, double label_temperature, int per_image,
                                 double *d_curve, double *d_rows, double *d_images, void *d_work, void *stream) {
    if (!d_pred || !d_label || !d_offsets || !temperatures || !d_curve || !d_rows || !d_images || !d_work) {
        fs_set_error("fs_map_list_sweep: null pointer");
        return FS_ERR_ARG;
    }
    for (const void *p : {(const void *)d_pred, (const void *)d_label, (const void *)d_offsets})
        if ((uintptr_t)p % 4) {
            fs_set_error("fs_map_list_sweep: float and int pointers must be 4-byte aligned");
            return FS_ERR_ARG;
        }
    for (const void *p : {(const void *)temperatures, (const void *)d_curve, (const void *)d_rows, (const void *)d_images,
                          (const void *)d_work})
        if ((uintptr_t)p % 8) {
            fs_set_error("fs_map_list_sweep: temperatures, d_curve, d_rows, d_images and d_work must be 8-byte aligned");
            return FS_ERR_ARG;
        }
    if (images < 1 || labels < 1) {
        fs_set_error("fs_map_list_sweep: images >= 1 and labels >= 1");
        return FS_ERR_ARG;
    }
    if (n_temperatures < 1 || n_temperatures > FS_MS_MAX_TEMPERATURES) {
        fs_set_error("fs_map_list_sweep: n_temperatures is 1 to 64");
        return FS_ERR_ARG;
    }
    if (per_image != 0 && per_image != 1) {
        fs_set_error("fs_map_list_sweep: per_image is 0 or 1");
        return FS_ERR_ARG;
    }
    fs_ms_betas betas;
    bool fine = fs_ms_positive(label_temperature) && fs_ms_positive(1.0 / label_temperature);
    for (int s = 0; s < FS_MS_MAX_TEMPERATURES; ++s) {
        betas.beta[s] = 0.0;
        if (s < n_temperatures) {
            fine = fine && fs_ms_positive(temperatures[s]) && fs_ms_positive(1.0 / temperatures[s]);
            betas.beta[s] = 1.0 / temperatures[s];
        }
    }
    if (!fine) {
        fs_set_error("fs_map_list_sweep: every temperature and label_temperature > 0, finite with finite reciprocals");
        return FS_ERR_ARG;
    }
    double *d_picked = (double *)d_work;
    hipLaunchKernelGGL(fs_k_map_sweep_image, dim3(images), dim3(FS_MS_THREADS), 0, (hipStream_t)stream, d_pred, d_label, d_offsets,
                       labels, betas, n_temperatures, label_temperature, d_rows, d_images, d_picked);
    if (!fs_hip_ok(hipGetLastError(), "fs_map_list_sweep image launch")) return FS_ERR_HIP;
    hipLaunchKernelGGL(fs_k_map_sweep_finish, dim3(n_temperatures), dim3(FS_MS_THREADS), 0, (hipStream_t)stream, d_offsets, images,
                       labels, n_temperatures, per_image, d_rows, d_images, d_picked, d_curve);
    return fs_hip_ok(hipGetLastError(), "fs_map_list_sweep finish launch") ? FS_OK : FS_ERR_HIP;
}
