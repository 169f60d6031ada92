// fs_vntrain.hip -- the three convolution passes of SpatialValueNet's 16 -> 16 layers for TRAINING (nets.Conv16Function):
//   fs_conv16_forward   y  = conv3x3(x, W)            stride 1, zero padding 1, no bias
//                       dx = conv3x3(g, W')           W'[ic][oc][tap] = W[oc][ic][8 - tap]   (transposed = 1: same kernel)
//   fs_conv16_wgrad     dW[oc][ic][ky][kx] = sum_{b,y,x} g[b,oc,y,x] x[b,ic,y+ky-1,x+kx-1]
// fp32, NCHW-contiguous, 64 x 64 maps, any batch >= 1; the weights are read on the device in PyTorch's own [16][16][3][3]
// layout, so a train step never copies them to the host.  BatchNorm in batch-statistics mode, the activations, the
// residual add, the loss, the first / last layer and Adam stay PyTorch operators (memory-bound passes).
//
// Why by hand: as GEMMs these layers are [pixels x 144] x [144 x 16]; the library's implicit-GEMM kernels pad N to 32.
// Like fs_valuenet.hip's block kernel, everything here runs on exact-fp32 MFMA (v_mfma_f32_16x16x4_f32) with N = 16.
// This file shares no code with fs_valuenet.hip: the inference kernels' ISA is untouched.
//
// fs_k_c16_conv (forward and data gradient): a workgroup (8 wavefronts) owns an 8-row strip of one image.  The strip plus
//   its one-row halo (10 rows, 16 channels) goes into LDS channel-planar -- row stride 72 floats (image column x at x + 4,
//   zero halo columns at 3 and 68), plane stride 720 = 16 (mod 32), so the four 16-lane channel groups of a wavefront read
//   disjoint banks.  M = 16 pixels of a row, N = 16 output channels, K = 4 input channels of a tap: 36 MFMAs per 16-pixel
//   tile, four row tiles per wavefront sharing the B operand.  The B operands are staged in LDS from W with the index map
//   of the pass (plain or transposed + flipped).  One tile per workgroup, the same instruction sequence for every image:
//   an image's result does not depend on what shares its launch.
// fs_k_c16_wgrad: M = oc, N = ic, K = 4 pixels, one accumulator tile per tap (9 x 4 registers).  A workgroup owns the
//   same 8-row strip; wavefront w owns row w.  x goes through LDS (each value is used by 3 rows x 3 columns; plane stride
//   772 = 4 (mod 64): a quarter-wave's float4 reads fall on distinct banks), g straight from global memory into registers
//   (each value is used once).  Lane (c, k) takes pixels 16 q + 4 k .. + 3 of its row for the four MFMAs of group q -- the
//   order of the K dimension is free as long as A and B agree.  The eight wavefronts' tiles are added in LDS in the fixed
//   order ((0+4)+(1+5))+((2+6)+(3+7)) and written to work[image * 8 + strip][oc][ic][tap].
// fs_k_c16_wgrad_reduce: dW[e] = the partials in a fixed order: eight contiguous slices of `batch` partials each are summed
//   front to back, the eight sums in a fixed tree.  No atomics anywhere: the same inputs give the same bits.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/flingsim.h"
#include "fs_context.h"

typedef float ct_f32x4 __attribute__((ext_vector_type(4)));

#define CT_W 64          // map width and height
#define CT_ROWS 8        // rows per strip
#define CT_STRIPS 8
#define CT_THREADS 512
#define CT_RS 72         // LDS row stride (floats)
#define CT_CS 720        // conv kernel: channel plane stride, 10 rows * 72 = 720 = 16 (mod 32)
#define CT_NT 4          // conv kernel: row tiles per wavefront
#define CT_XS 772        // wgrad kernel: channel plane stride, >= 720 and = 4 (mod 64)
#define CT_DW 2304       // 16 * 16 * 9

// workgroup id -> (image, strip) with the eight strips of an image on one XCD (workgroup n runs on XCD n % 8)
__device__ __forceinline__ bool ct_tile_of(int n, int batch, int &image, int &strip) {
    const int xcd = n & 7, k = n >> 3;
    image = (k / CT_STRIPS) * 8 + xcd;
    strip = k % CT_STRIPS;
    return image < batch;
}

// rows y0 - 1 .. y0 + 8 of the 16 channels of image b -> LDS planes of stride CS, zero outside the image, zero halo columns
template <int CS>
__device__ __forceinline__ void ct_stage_tile(const float *__restrict__ in, int b, int y0, int t, float *s) {
    const float *src = in + (size_t)b * 16 * CT_W * CT_W;
#pragma unroll
    for (int k = 0; k < 5; ++k) {   // 16 channels * 10 rows * 16 float4 = 2560 = 5 * 512
        const int idx = t + CT_THREADS * k, ch = idx / 160, rem = idx % 160, r = rem >> 4, q = rem & 15, y = y0 - 1 + r;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if ((unsigned)y < (unsigned)CT_W) v = *(const float4 *)(src + ((size_t)ch * CT_W + y) * CT_W + 4 * q);
        *(float4 *)(s + ch * CS + r * CT_RS + 4 + 4 * q) = v;
    }
    if (t < 16 * 20) {
        const int ch = t / 20, rem = t % 20;
        s[ch * CS + (rem >> 1) * CT_RS + ((rem & 1) ? 68 : 3)] = 0.f;
    }
}

// ---- forward / data gradient ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(CT_THREADS) void fs_k_c16_conv(const float *__restrict__ W, const float *__restrict__ in,
                                                            int transposed, int batch, float *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) float s_in[16 * CT_CS];
    __shared__ float s_w[36 * 64];
    int b, strip;
    if (!ct_tile_of(blockIdx.x, batch, b, strip)) return;
    const int t = threadIdx.x, l = t & 63, wv = t >> 6, y0 = strip * CT_ROWS;
    ct_stage_tile<CT_CS>(in, b, y0, t, s_in);
    // B operand of k-step s = tap * 4 + cg, lane l: Wm[n = l & 15][k = 4 cg + (l >> 4)][tap], where Wm is W itself or, for
    // the data gradient, Wm[n][k][tap] = W[k][n][8 - tap]
    for (int i = t; i < 36 * 64; i += CT_THREADS) {
        const int s = i >> 6, ln = i & 63, tap = s >> 2, cg = s & 3, n = ln & 15, k = 4 * cg + (ln >> 4);
        s_w[i] = transposed ? W[(k * 16 + n) * 9 + 8 - tap] : W[(n * 16 + k) * 9 + tap];
    }
    __syncthreads();
    const int oc = l & 15, kg = l >> 4, xt = wv & 3, rpar = wv >> 2;
    const float *a = s_in + kg * CT_CS + rpar * CT_RS + xt * 16 + (l & 15) + 3;   // A[m = l & 15][k = l >> 4]
    const float *w = s_w + l;
    ct_f32x4 acc[CT_NT];
#pragma unroll
    for (int j = 0; j < CT_NT; ++j) acc[j] = (ct_f32x4){0.f, 0.f, 0.f, 0.f};
    // A operands one filter tap (4 channel groups x CT_NT tiles) ahead of the MFMAs that consume them
    float cur[4][CT_NT], nxt[4][CT_NT];
#pragma unroll
    for (int cg = 0; cg < 4; ++cg)
#pragma unroll
        for (int j = 0; j < CT_NT; ++j) cur[cg][j] = a[cg * 4 * CT_CS + j * 2 * CT_RS];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        float wt[4];
#pragma unroll
        for (int cg = 0; cg < 4; ++cg) wt[cg] = w[(tap * 4 + cg) * 64];
        if (tap < 8) {
            const int off = ((tap + 1) / 3) * CT_RS + ((tap + 1) % 3);
#pragma unroll
            for (int cg = 0; cg < 4; ++cg)
#pragma unroll
                for (int j = 0; j < CT_NT; ++j) nxt[cg][j] = a[off + cg * 4 * CT_CS + j * 2 * CT_RS];
        }
#pragma unroll
        for (int cg = 0; cg < 4; ++cg)
#pragma unroll
            for (int j = 0; j < CT_NT; ++j)
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur[cg][j], wt[cg], acc[j], 0, 0, 0);
#pragma unroll
        for (int cg = 0; cg < 4; ++cg)
#pragma unroll
            for (int j = 0; j < CT_NT; ++j) cur[cg][j] = nxt[cg][j];
    }
    // D[m = 4 (l >> 4) + i][n = l & 15]: four neighbouring pixels of channel oc
    float *dst = out + ((size_t)b * 16 + oc) * CT_W * CT_W + xt * 16 + 4 * kg;
#pragma unroll
    for (int j = 0; j < CT_NT; ++j) *(ct_f32x4 *)(dst + (size_t)(y0 + rpar + 2 * j) * CT_W) = acc[j];
}

// ---- weight gradient: per-strip partial tiles ----------------------------------------------------------------------------
__global__ __launch_bounds__(CT_THREADS) void fs_k_c16_wgrad(const float *__restrict__ x, const float *__restrict__ g,
                                                             int batch, float *__restrict__ work) {
    __shared__ __attribute__((aligned(16))) float s_x[16 * CT_XS];   // later: four wavefronts' accumulator tiles
    int b, strip;
    if (!ct_tile_of(blockIdx.x, batch, b, strip)) return;
    const int t = threadIdx.x, l = t & 63, wv = t >> 6, y0 = strip * CT_ROWS;
    const int c = l & 15, kk = l >> 4;
    // A[m = oc = c][k = kk]: this lane's 16 values of g's row y0 + wv, requested before the x tile is staged
    const float *grow = g + (((size_t)b * 16 + c) * CT_W + y0 + wv) * CT_W + 4 * kk;
    ct_f32x4 gv[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) gv[q] = *(const ct_f32x4 *)(grow + 16 * q);
    ct_stage_tile<CT_XS>(x, b, y0, t, s_x);
    __syncthreads();
    ct_f32x4 acc[9];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) acc[tap] = (ct_f32x4){0.f, 0.f, 0.f, 0.f};
    // B[k = kk][n = ic = c]: tile row wv + ky is image row y0 + wv + ky - 1; column p lives at p + 4
    const float *xb = s_x + c * CT_XS + wv * CT_RS + 4 + 4 * kk;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float xs[3][6];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const float *p = xb + ky * CT_RS + 16 * q;
            const ct_f32x4 m = *(const ct_f32x4 *)p;
            xs[ky][0] = p[-1];
            xs[ky][1] = m[0]; xs[ky][2] = m[1]; xs[ky][3] = m[2]; xs[ky][4] = m[3];
            xs[ky][5] = p[4];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx)
                    acc[ky * 3 + kx] = __builtin_amdgcn_mfma_f32_16x16x4f32(gv[q][j], xs[ky][j + kx], acc[ky * 3 + kx], 0, 0, 0);
    }
    // D[m = oc = 4 kk + i][n = ic = c] of tap -> element ((4 kk + i) * 16 + c) * 9 + tap.  Wavefronts 4..7 hand their tiles
    // to 0..3, then 0..3 publish theirs and all threads add the four in a fixed tree.
    float *s_r = s_x;
    const int e0 = (4 * kk * 16 + c) * 9;
    __syncthreads();   // every wavefront is done with the x tile
    if (wv >= 4) {
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
#pragma unroll
            for (int i = 0; i < 4; ++i) s_r[(wv - 4) * CT_DW + e0 + i * 144 + tap] = acc[tap][i];
    }
    __syncthreads();
    if (wv < 4) {
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[tap][i] = acc[tap][i] + s_r[wv * CT_DW + e0 + i * 144 + tap];
    }
    __syncthreads();
    if (wv < 4) {
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
#pragma unroll
            for (int i = 0; i < 4; ++i) s_r[wv * CT_DW + e0 + i * 144 + tap] = acc[tap][i];
    }
    __syncthreads();
    float *dst = work + ((size_t)b * CT_STRIPS + strip) * CT_DW;
    for (int e = t; e < CT_DW; e += CT_THREADS)
        dst[e] = (s_r[e] + s_r[CT_DW + e]) + (s_r[2 * CT_DW + e] + s_r[3 * CT_DW + e]);
}

// ---- weight gradient: the partials in a fixed order ---------------------------------------------------------------------
// 256 threads = 32 elements x 8 slices; slice s holds partials s * batch .. (s + 1) * batch - 1 (there are 8 * batch)
__global__ __launch_bounds__(256) void fs_k_c16_wgrad_reduce(const float *__restrict__ work, int batch, float *__restrict__ dw) {
    __shared__ float s[8][32];
    const int t = threadIdx.x, el = t & 31, sl = t >> 5, e = blockIdx.x * 32 + el;
    const float *src = work + (size_t)sl * batch * CT_DW + e;
    float sum = 0.f;
#pragma unroll 8   // eight loads in flight; the additions keep their order
    for (int p = 0; p < batch; ++p) sum = sum + src[(size_t)p * CT_DW];
    s[sl][el] = sum;
    __syncthreads();
    if (sl == 0)
        dw[e] = ((s[0][el] + s[1][el]) + (s[2][el] + s[3][el])) + ((s[4][el] + s[5][el]) + (s[6][el] + s[7][el]));
}

// ---- C-ABI -----------------------------------------------------------------------------------------------------------
extern "C" {

size_t fs_conv16_work_bytes(int batch, int dim) {
    if (batch < 1 || dim != CT_W) return 0;
    return (size_t)batch * CT_STRIPS * CT_DW * sizeof(float);
}

int fs_conv16_forward(const float *d_x, const float *d_w, int transposed, int batch, int dim, float *d_y, void *stream) {
    if (!d_x || !d_w || !d_y || batch < 1 || dim != CT_W || (transposed != 0 && transposed != 1)) {
        fs_set_error("fs_conv16_forward: bad arguments (the kernels are built for [batch >= 1][16][64][64])");
        return FS_ERR_ARG;
    }
    if (fs_misaligned16({d_x, d_w, d_y})) {   // moved as float4
        fs_set_error("fs_conv16_forward: d_x, d_w and d_y must be 16-byte aligned");
        return FS_ERR_ARG;
    }
    if (d_x == d_y) {
        fs_set_error("fs_conv16_forward: in place is not supported (strips read their neighbours' rows)");
        return FS_ERR_ARG;
    }
    const int grid = ((batch + 7) / 8) * 8 * CT_STRIPS;
    hipLaunchKernelGGL(fs_k_c16_conv, dim3(grid), dim3(CT_THREADS), 0, (hipStream_t)stream, d_w, d_x, transposed, batch, d_y);
    return fs_hip_ok(hipGetLastError(), "fs_conv16_forward launch") ? FS_OK : FS_ERR_HIP;
}

int fs_conv16_wgrad(const float *d_x, const float *d_g, int batch, int dim, float *d_dw, void *d_work, void *stream) {
    if (!d_x || !d_g || !d_dw || !d_work || batch < 1 || dim != CT_W) {
        fs_set_error("fs_conv16_wgrad: bad arguments (the kernels are built for [batch >= 1][16][64][64])");
        return FS_ERR_ARG;
    }
    if (fs_misaligned16({d_x, d_g, d_dw, d_work})) {
        fs_set_error("fs_conv16_wgrad: d_x, d_g, d_dw and d_work must be 16-byte aligned");
        return FS_ERR_ARG;
    }
    const int grid = ((batch + 7) / 8) * 8 * CT_STRIPS;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(fs_k_c16_wgrad, dim3(grid), dim3(CT_THREADS), 0, st, d_x, d_g, batch, (float *)d_work);
    hipLaunchKernelGGL(fs_k_c16_wgrad_reduce, dim3(CT_DW / 32), dim3(256), 0, st, (const float *)d_work, batch, d_dw);
    return fs_hip_ok(hipGetLastError(), "fs_conv16_wgrad launch") ? FS_OK : FS_ERR_HIP;
}

}  // extern "C"
