// fs_bntrain.hip -- BatchNorm2d(16) in batch-statistics (training) mode with its activation and residual add fused, forward and
// backward, for SpatialValueNet's 17 BatchNorm sites (nets.BatchNormAct16Function):
//   fs_bn16_forward    mean_c = sum x / N, var_c = sum (x - mean_c)^2 / N (biased), invstd_c = 1 / sqrt(var_c + eps), N = batch * 4096
//                      z = (x - mean_c) * invstd_c * gamma_c + beta_c (+ residual),   y = z > 0 ? z : slope * z
//   fs_bn16_backward   dz = dy * (y > 0 ? 1 : slope)   -- the mask is read from the stored forward output, never recomputed
//                      dbeta_c = sum dz, dgamma_c = sum dz * xh, xh = (x - mean_c) * invstd_c
//                      dx = gamma_c * invstd_c * (dz - dbeta_c / N - xh * dgamma_c / N),   dresidual = dz
// fp32, NCHW-contiguous, 64 x 64 maps, any batch >= 1: the conventions of fs_vntrain.hip, with which this file shares no code.
// slope = 0 is ReLU, 0.01 the first layer's LeakyReLU, 1 no activation (then y is not read by the backward).
//
// Why by hand: a library BatchNorm splits the work by channel, and 16 channels cannot fill 256 CUs.  Here the unit of work is
// one 16 KiB plane (image b, channel c): batch * 16 workgroups of 256 threads, four float4 per thread and tensor.
//   pass 1 (fs_k_bn16_stats / fs_k_bn16_bwd_reduce): every plane's two sums -> work[c][b] as a double2.
//   pass 2 (fs_k_bn16_fwd_apply / fs_k_bn16_bwd_apply): every wavefront first adds the `batch` partials of its channel -- lane l
//     takes partials l, l + 64, ... front to back, then a 6-step xor butterfly, so all lanes of all workgroups hold the same bits
//     without LDS, a barrier or a third launch -- while its own loads of the plane are in flight; then one streaming pass.
//     The workgroup of image 0 writes the per-channel outputs (save_mean / save_invstd / running statistics; dgamma / dbeta).
// Statistics are accumulated in float64: a plane's sums are taken about its first element K (sum (x - K), sum (x - K)^2, exact
// differences), turned into (mean_p, M2_p) and merged as equal-count groups, M2 = sum_p M2_p + 4096 (mean_p - mean)^2.  A channel
// whose mean is 10^4 times its spread keeps its variance, a constant channel has mean exactly its value and variance exactly 0.
// No atomics and no arrival counters anywhere: every sum has a fixed order, the same inputs give the same bits.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/flingsim.h"
#include "fs_context.h"

#define BN_C 16
#define BN_PLANE 4096    // 64 * 64
#define BN_THREADS 256
#define BN_V 4           // float4 per thread and plane: 4 * 256 * 4 = 4096

// a + the same value of the 63 other lanes, in a fixed order; every lane gets the same bits (each step adds the same two numbers)
__device__ __forceinline__ double bn_wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
    return v;
}

// the four wavefronts' sums of (a, q): ((w0 + w1) + (w2 + w3)) in every thread
__device__ __forceinline__ void bn_block_sum2(double &a, double &q, double (*s)[4]) {
    a = bn_wave_sum(a);
    q = bn_wave_sum(q);
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s[0][wv] = a; s[1][wv] = q; }
    __syncthreads();
    a = (s[0][0] + s[0][1]) + (s[0][2] + s[0][3]);
    q = (s[1][0] + s[1][1]) + (s[1][2] + s[1][3]);
}

__device__ __forceinline__ void bn_load_plane(const float *__restrict__ src, int t, float4 *v) {
#pragma unroll
    for (int k = 0; k < BN_V; ++k) v[k] = ((const float4 *)src)[t + BN_THREADS * k];
}

// the two per-channel sums over work[c][0 .. batch - 1] (x and y components), identical in every lane
__device__ __forceinline__ void bn_channel_sum2(const double2 *__restrict__ pc, int batch, double &a, double &q) {
    a = 0.0; q = 0.0;
    for (int p = threadIdx.x & 63; p < batch; p += 64) { const double2 v = pc[p]; a = a + v.x; q = q + v.y; }
    a = bn_wave_sum(a);
    q = bn_wave_sum(q);
}

// ---- forward, pass 1: (mean_p, M2_p) of every plane ------------------------------------------------------------------------
__global__ __launch_bounds__(BN_THREADS) void fs_k_bn16_stats(const float *__restrict__ x, int batch, double2 *__restrict__ part) {
    __shared__ double s[2][4];
    const int t = threadIdx.x, b = blockIdx.x >> 4, c = blockIdx.x & 15;
    const float *src = x + (size_t)blockIdx.x * BN_PLANE;
    float4 v[BN_V];
    bn_load_plane(src, t, v);
    const double K = (double)src[0];
    double a = 0.0, q = 0.0;
#pragma unroll
    for (int k = 0; k < BN_V; ++k) {
        const float e[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
#pragma unroll
        for (int i = 0; i < 4; ++i) { const double d = (double)e[i] - K; a = a + d; q = q + d * d; }
    }
    bn_block_sum2(a, q, s);
    if (t == 0) {
        const double m2 = q - a * a / (double)BN_PLANE;
        part[(size_t)c * batch + b] = make_double2(K + a / (double)BN_PLANE, m2 > 0.0 ? m2 : 0.0);
    }
}

// ---- forward, pass 2 ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BN_THREADS) void fs_k_bn16_fwd_apply(const float *__restrict__ x, const float *__restrict__ res,
                                                                  const float *__restrict__ gamma, const float *__restrict__ beta,
                                                                  const double2 *__restrict__ part, int batch, float eps, float slope,
                                                                  float momentum, float *running_mean, float *running_var,
                                                                  float *__restrict__ y, float *__restrict__ save_mean,
                                                                  float *__restrict__ save_invstd) {
    const int t = threadIdx.x, b = blockIdx.x >> 4, c = blockIdx.x & 15;
    const size_t base = (size_t)blockIdx.x * BN_PLANE;
    float4 v[BN_V], r[BN_V];
    bn_load_plane(x + base, t, v);
    if (res) bn_load_plane(res + base, t, r);
    // the channel's statistics out of the planes' (two sweeps over `batch` partials; the second is served by the cache)
    const double2 *pc = part + (size_t)c * batch;
    const int l = t & 63;
    double sm = 0.0;
    for (int p = l; p < batch; p += 64) sm = sm + pc[p].x;
    const double mean = bn_wave_sum(sm) / (double)batch;
    double m2 = 0.0;
    for (int p = l; p < batch; p += 64) { const double2 pp = pc[p]; const double d = pp.x - mean; m2 = m2 + (pp.y + (double)BN_PLANE * (d * d)); }
    const double n = (double)batch * (double)BN_PLANE;
    const double var = bn_wave_sum(m2) / n;
    const float mean_f = (float)mean, invstd_f = (float)(1.0 / sqrt(var + (double)eps));
    if (b == 0 && t == 0) {
        save_mean[c] = mean_f;
        save_invstd[c] = invstd_f;
        if (running_mean) {
            running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mean_f;
            running_var[c] = (1.f - momentum) * running_var[c] + momentum * (float)(var * n / (n - 1.0));
        }
    }
    const float g = gamma[c], bt = beta[c];
#pragma unroll
    for (int k = 0; k < BN_V; ++k) {
        const float e[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
        float rr[4] = {0.f, 0.f, 0.f, 0.f}, o[4];
        if (res) { rr[0] = r[k].x; rr[1] = r[k].y; rr[2] = r[k].z; rr[3] = r[k].w; }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float z = (e[i] - mean_f) * invstd_f * g + bt;
            if (res) z = z + rr[i];
            o[i] = z > 0.f ? z : slope * z;
        }
        ((float4 *)(y + base))[t + BN_THREADS * k] = make_float4(o[0], o[1], o[2], o[3]);
    }
}

// ---- backward, pass 1: (sum dz, sum dz * xh) of every plane ------------------------------------------------------------------
__global__ __launch_bounds__(BN_THREADS) void fs_k_bn16_bwd_reduce(const float *__restrict__ x, const float *__restrict__ y,
                                                                   const float *__restrict__ dy, const float *__restrict__ save_mean,
                                                                   const float *__restrict__ save_invstd, float slope, int batch,
                                                                   double2 *__restrict__ part) {
    __shared__ double s[2][4];
    const int t = threadIdx.x, b = blockIdx.x >> 4, c = blockIdx.x & 15;
    const size_t base = (size_t)blockIdx.x * BN_PLANE;
    const bool masked = slope != 1.f;   // slope 1: the factor is 1 wherever y lies
    float4 v[BN_V], o[BN_V], g[BN_V];
    bn_load_plane(x + base, t, v);
    bn_load_plane(dy + base, t, g);
    if (masked) bn_load_plane(y + base, t, o);
    const float mean = save_mean[c], invstd = save_invstd[c];
    double a = 0.0, q = 0.0;
#pragma unroll
    for (int k = 0; k < BN_V; ++k) {
        const float e[4] = {v[k].x, v[k].y, v[k].z, v[k].w}, d[4] = {g[k].x, g[k].y, g[k].z, g[k].w};
        float f[4] = {1.f, 1.f, 1.f, 1.f};
        if (masked) { f[0] = o[k].x > 0.f ? 1.f : slope; f[1] = o[k].y > 0.f ? 1.f : slope; f[2] = o[k].z > 0.f ? 1.f : slope; f[3] = o[k].w > 0.f ? 1.f : slope; }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float dz = d[i] * f[i], xh = (e[i] - mean) * invstd;
            a = a + (double)dz;
            q = q + (double)dz * (double)xh;
        }
    }
    bn_block_sum2(a, q, s);
    if (t == 0) part[(size_t)c * batch + b] = make_double2(a, q);
}

// ---- backward, pass 2 -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BN_THREADS) void fs_k_bn16_bwd_apply(const float *__restrict__ x, const float *__restrict__ y,
                                                                  const float *__restrict__ dy, const float *__restrict__ gamma,
                                                                  const float *__restrict__ save_mean, const float *__restrict__ save_invstd,
                                                                  const double2 *__restrict__ part, float slope, int batch,
                                                                  float *__restrict__ dx, float *__restrict__ dres,
                                                                  float *__restrict__ dgamma, float *__restrict__ dbeta) {
    const int t = threadIdx.x, b = blockIdx.x >> 4, c = blockIdx.x & 15;
    const size_t base = (size_t)blockIdx.x * BN_PLANE;
    const bool masked = slope != 1.f;
    float4 v[BN_V], o[BN_V], g[BN_V];
    bn_load_plane(x + base, t, v);
    bn_load_plane(dy + base, t, g);
    if (masked) bn_load_plane(y + base, t, o);
    double sb, sg;
    bn_channel_sum2(part + (size_t)c * batch, batch, sb, sg);
    const double n = (double)batch * (double)BN_PLANE;
    const float k1 = (float)(sb / n), k2 = (float)(sg / n);
    const float mean = save_mean[c], invstd = save_invstd[c], gi = gamma[c] * invstd;
    if (b == 0 && t == 0) { dbeta[c] = (float)sb; dgamma[c] = (float)sg; }
#pragma unroll
    for (int k = 0; k < BN_V; ++k) {
        const float e[4] = {v[k].x, v[k].y, v[k].z, v[k].w}, d[4] = {g[k].x, g[k].y, g[k].z, g[k].w};
        float f[4] = {1.f, 1.f, 1.f, 1.f}, dz[4], out[4];
        if (masked) { f[0] = o[k].x > 0.f ? 1.f : slope; f[1] = o[k].y > 0.f ? 1.f : slope; f[2] = o[k].z > 0.f ? 1.f : slope; f[3] = o[k].w > 0.f ? 1.f : slope; }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            dz[i] = d[i] * f[i];
            const float xh = (e[i] - mean) * invstd;
            out[i] = gi * (dz[i] - k1 - xh * k2);
        }
        ((float4 *)(dx + base))[t + BN_THREADS * k] = make_float4(out[0], out[1], out[2], out[3]);
        if (dres) ((float4 *)(dres + base))[t + BN_THREADS * k] = make_float4(dz[0], dz[1], dz[2], dz[3]);
    }
}

// ---- C-ABI -----------------------------------------------------------------------------------------------------------
extern "C" {

size_t fs_bn16_work_bytes(int batch, int dim) {
    if (batch < 1 || dim != 64) return 0;
    return (size_t)batch * BN_C * sizeof(double2);
}

int fs_bn16_forward(const float *d_x, const float *d_residual, const float *d_gamma, const float *d_beta, float eps, float slope,
                    float momentum, float *d_running_mean, float *d_running_var, int batch, int dim, float *d_y, float *d_save_mean,
                    float *d_save_invstd, void *d_work, void *stream) {
    if (!d_x || !d_gamma || !d_beta || !d_y || !d_save_mean || !d_save_invstd || !d_work || batch < 1 || dim != 64) {
        fs_set_error("fs_bn16_forward: bad arguments (the kernels are built for [batch >= 1][16][64][64])");
        return FS_ERR_ARG;
    }
    if ((d_running_mean == nullptr) != (d_running_var == nullptr)) {
        fs_set_error("fs_bn16_forward: d_running_mean and d_running_var are given together or not at all");
        return FS_ERR_ARG;
    }
    if (fs_misaligned16({d_x, d_residual, d_gamma, d_beta, d_running_mean, d_running_var, d_y, d_save_mean, d_save_invstd, d_work})) {
        fs_set_error("fs_bn16_forward: every pointer must be 16-byte aligned");
        return FS_ERR_ARG;
    }
    if (d_x == d_y) {
        fs_set_error("fs_bn16_forward: in place is not supported (d_y == d_x)");
        return FS_ERR_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)batch * BN_C), block(BN_THREADS);
    hipLaunchKernelGGL(fs_k_bn16_stats, grid, block, 0, st, d_x, batch, (double2 *)d_work);
    hipLaunchKernelGGL(fs_k_bn16_fwd_apply, grid, block, 0, st, d_x, d_residual, d_gamma, d_beta, (const double2 *)d_work, batch, eps,
                       slope, momentum, d_running_mean, d_running_var, d_y, d_save_mean, d_save_invstd);
    return fs_hip_ok(hipGetLastError(), "fs_bn16_forward launch") ? FS_OK : FS_ERR_HIP;
}

int fs_bn16_backward(const float *d_x, const float *d_y, const float *d_dy, const float *d_gamma, const float *d_save_mean,
                     const float *d_save_invstd, float slope, int batch, int dim, float *d_dx, float *d_dresidual, float *d_dgamma,
                     float *d_dbeta, void *d_work, void *stream) {
    if (!d_x || !d_y || !d_dy || !d_gamma || !d_save_mean || !d_save_invstd || !d_dx || !d_dgamma || !d_dbeta || !d_work || batch < 1 ||
        dim != 64) {
        fs_set_error("fs_bn16_backward: bad arguments (the kernels are built for [batch >= 1][16][64][64])");
        return FS_ERR_ARG;
    }
    if (fs_misaligned16({d_x, d_y, d_dy, d_gamma, d_save_mean, d_save_invstd, d_dx, d_dresidual, d_dgamma, d_dbeta, d_work})) {
        fs_set_error("fs_bn16_backward: every pointer must be 16-byte aligned");
        return FS_ERR_ARG;
    }
    if (d_dx == d_dy) {
        fs_set_error("fs_bn16_backward: in place is not supported (d_dx == d_dy)");
        return FS_ERR_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)batch * BN_C), block(BN_THREADS);
    hipLaunchKernelGGL(fs_k_bn16_bwd_reduce, grid, block, 0, st, d_x, d_y, d_dy, d_save_mean, d_save_invstd, slope, batch,
                       (double2 *)d_work);
    hipLaunchKernelGGL(fs_k_bn16_bwd_apply, grid, block, 0, st, d_x, d_y, d_dy, d_gamma, d_save_mean, d_save_invstd,
                       (const double2 *)d_work, slope, batch, d_dx, d_dresidual, d_dgamma, d_dbeta);
    return fs_hip_ok(hipGetLastError(), "fs_bn16_backward launch") ? FS_OK : FS_ERR_HIP;
}

}  // extern "C"
