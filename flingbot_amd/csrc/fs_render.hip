// fs_render.hip -- vertex normals, coverage reward and the software rasteriser of libflingsim.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/flingsim.h"
#include "fs_context.h"
#include "fs_raster_kernels.h"

#define HIP_TRY(call)                                     \
    do {                                                  \
        if (!fs_hip_ok((call), #call)) return FS_ERR_HIP; \
    } while (0)

// ---------------------------------------------------------------------------------------------------------------
// Vertex normals: area-weighted sum of incident triangle normals, normalised, fallback (0,1,0).
// Same formula as the reference's host code (main.cpp:904-919) and what NvFlexGetNormals returns (main.cpp:2286).
// Gather over the vertex->triangle CSR in ascending triangle id = the accumulation order of a sequential loop over
// triangles, so the result is deterministic.
__global__ __launch_bounds__(256) void fs_k_vertex_normals(const FsVec4 *__restrict__ pos, const int *__restrict__ tris,
                                                           const int *__restrict__ vt_off,
                                                           const int *__restrict__ vt_tri, FsVec4 *__restrict__ nrm, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    for (int q = vt_off[i]; q < vt_off[i + 1]; ++q) {
        const int t = vt_tri[q];
        const FsVec4 v0 = pos[tris[3 * t]], v1 = pos[tris[3 * t + 1]], v2 = pos[tris[3 * t + 2]];
        float ax = v1.x - v0.x, ay = v1.y - v0.y, az = v1.z - v0.z;
        float bx = v2.x - v0.x, by = v2.y - v0.y, bz = v2.z - v0.z;
        sx += ay * bz - az * by;
        sy += az * bx - ax * bz;
        sz += ax * by - ay * bx;
    }
    float l = sx * sx + sy * sy + sz * sz;
    FsVec4 o;
    if (l > 0.0f) {
        float inv = 1.0f / sqrtf(l);
        o = FsVec4{sx * inv, sy * inv, sz * inv, 0.0f};
    } else {
        o = FsVec4{0.0f, 1.0f, 0.0f, 0.0f};
    }
    nrm[i] = o;
}

static int ensure_scratch(fs_ctx *ctx, size_t bytes) {
    if (bytes <= ctx->render_scratch_bytes) return FS_OK;
    if (ctx->render_scratch) (void)hipFree(ctx->render_scratch);
    ctx->render_scratch = nullptr;
    ctx->render_scratch_bytes = 0;
    HIP_TRY(hipMalloc(&ctx->render_scratch, bytes));
    ctx->render_scratch_bytes = bytes;
    return FS_OK;
}

// normals of env into device buffer `d_nrm` (float4[n])
static int launch_normals(fs_ctx *ctx, const FsEnv &e, FsVec4 *d_nrm) {
    const int n = e.host.n;
    hipLaunchKernelGGL(fs_k_vertex_normals, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, e.dev.pos, e.topo->tris,
                       e.topo->vt_off, e.topo->vt_tri, d_nrm, n);
    HIP_TRY(hipGetLastError());
    return FS_OK;
}

int fs_normals_env(fs_ctx *ctx, int env, float *out4n) {
    FsEnv &e = ctx->envs[env];
    const size_t bytes = size_t(16) * e.host.n;
    int rc = ensure_scratch(ctx, bytes);
    if (rc != FS_OK) return rc;
    rc = launch_normals(ctx, e, (FsVec4 *)ctx->render_scratch);
    if (rc != FS_OK) return rc;
    void *st = fs_stage(ctx, bytes);
    if (!st) return FS_ERR_HIP;
    HIP_TRY(hipMemcpyAsync(st, ctx->render_scratch, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    memcpy(out4n, st, bytes);
    return FS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Coverage reward (reference environment/flex_utils.py:358-395, pos=None path => float32 positions):
//   bbox of (x, z); span = extent / 100 (fp32); per particle the slots round((offset -/+ r) / span) clipped to
//   [0, 100]; vectorized_range(start, end) samples floor(k * (end - start) / N + start), k < N = max(end - start) + 1
//   (fp64); cells idx = x * 100 + y clipped to [0, 9999]; area = #cells * span_x * span_y (fp64).
// One workgroup per episode; the 100x100 occupancy grid lives in LDS.
// np.min / np.max propagate NaN (fminf / fmaxf drop it): one NaN x or z makes the span, and so the reference's area, NaN.
__device__ __forceinline__ float fs_cov_min(float a, float b) { return (a != a || b != b) ? __int_as_float(0x7fc00000) : fminf(a, b); }
__device__ __forceinline__ float fs_cov_max(float a, float b) { return (a != a || b != b) ? __int_as_float(0x7fc00000) : fmaxf(a, b); }
__device__ __forceinline__ float fs_wave_min(float v) {
    for (int off = 32; off > 0; off >>= 1) v = fs_cov_min(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ float fs_wave_max(float v) {
    for (int off = 32; off > 0; off >>= 1) v = fs_cov_max(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ int fs_wave_max_i(int v) {
    for (int off = 32; off > 0; off >>= 1) { int o = __shfl_xor(v, off, 64); v = o > v ? o : v; }
    return v;
}

#define FS_COV_THREADS 1024  // one workgroup per episode: 16 waves go through the three passes over the particles
__global__ __launch_bounds__(FS_COV_THREADS) void fs_k_coverage(const FsEnvDev *envs, double *out, float particle_radius) {
    const FsEnvDev &E = envs[blockIdx.x];
    __shared__ unsigned char grid[10000];
    __shared__ float red[4][FS_COV_THREADS / 64];
    __shared__ int redi[2][FS_COV_THREADS / 64];
    __shared__ int total;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (!E.has_scene || E.n <= 0) {
        if (t == 0) out[blockIdx.x] = 0.0;
        return;
    }
    const int n = E.n;
    float mnx = 3.402823466e+38f, mnz = 3.402823466e+38f, mxx = -3.402823466e+38f, mxz = -3.402823466e+38f;
    for (int i = t; i < n; i += FS_COV_THREADS) {
        const FsVec4 p = E.pos[i];
        mnx = fs_cov_min(mnx, p.x); mxx = fs_cov_max(mxx, p.x);
        mnz = fs_cov_min(mnz, p.z); mxz = fs_cov_max(mxz, p.z);
    }
    mnx = fs_wave_min(mnx); mnz = fs_wave_min(mnz); mxx = fs_wave_max(mxx); mxz = fs_wave_max(mxz);
    if (lane == 0) { red[0][wave] = mnx; red[1][wave] = mnz; red[2][wave] = mxx; red[3][wave] = mxz; }
    for (int q = t; q < 10000; q += FS_COV_THREADS) grid[q] = 0;
    if (t == 0) total = 0;
    __syncthreads();
    for (int w = 0; w < FS_COV_THREADS / 64; ++w) {  // (min / max: the order of the reduction cannot change the result)
        mnx = fs_cov_min(mnx, red[0][w]); mnz = fs_cov_min(mnz, red[1][w]);
        mxx = fs_cov_max(mxx, red[2][w]); mxz = fs_cov_max(mxz, red[3][w]);
    }
    const float span0 = (mxx - mnx) / 100.0f, span1 = (mxz - mnz) / 100.0f;
    if (span0 != span0 || span1 != span1) {  // (the same for every thread) no slot is defined: the reference marks nothing, 0 * NaN
        if (t == 0) out[blockIdx.x] = (double)span0 * (double)span1;
        return;
    }
    // pass A: N = max(end - start) + 1 per axis
    int ex = -2147483647, ez = -2147483647;
    for (int i = t; i < n; i += FS_COV_THREADS) {
        const FsVec4 p = E.pos[i];
        const float ox = p.x - mnx, oz = p.z - mnz;
        long long xl = (long long)rintf((ox - particle_radius) / span0), xh = (long long)rintf((ox + particle_radius) / span0);
        long long zl = (long long)rintf((oz - particle_radius) / span1), zh = (long long)rintf((oz + particle_radius) / span1);
        if (xl < 0) xl = 0; if (xh > 100) xh = 100; if (zl < 0) zl = 0; if (zh > 100) zh = 100;
        int dx = (int)(xh - xl), dz = (int)(zh - zl);
        ex = dx > ex ? dx : ex; ez = dz > ez ? dz : ez;
    }
    ex = fs_wave_max_i(ex); ez = fs_wave_max_i(ez);
    if (lane == 0) { redi[0][wave] = ex; redi[1][wave] = ez; }
    __syncthreads();
    for (int w = 0; w < FS_COV_THREADS / 64; ++w) { ex = redi[0][w] > ex ? redi[0][w] : ex; ez = redi[1][w] > ez ? redi[1][w] : ez; }
    const int Nx = ex + 1, Nz = ez + 1;
    // pass B: mark cells
    for (int i = t; i < n; i += FS_COV_THREADS) {
        const FsVec4 p = E.pos[i];
        const float ox = p.x - mnx, oz = p.z - mnz;
        long long xl = (long long)rintf((ox - particle_radius) / span0), xh = (long long)rintf((ox + particle_radius) / span0);
        long long zl = (long long)rintf((oz - particle_radius) / span1), zh = (long long)rintf((oz + particle_radius) / span1);
        if (xl < 0) xl = 0; if (xh > 100) xh = 100; if (zl < 0) zl = 0; if (zh > 100) zh = 100;
        for (int kz = 0; kz < Nz; ++kz) {
            const long long iz = (long long)floor((double)(kz * (zh - zl)) / (double)Nz + (double)zl);
            for (int kx = 0; kx < Nx; ++kx) {
                const long long ix = (long long)floor((double)(kx * (xh - xl)) / (double)Nx + (double)xl);
                long long idx = ix * 100 + iz;
                idx = idx < 0 ? 0 : (idx > 9999 ? 9999 : idx);
                grid[idx] = 1;
            }
        }
    }
    __syncthreads();
    int cnt = 0;
    for (int q = t; q < 10000; q += FS_COV_THREADS) cnt += grid[q];
    atomicAdd(&total, cnt);
    __syncthreads();
    if (t == 0) out[blockIdx.x] = (double)total * (double)span0 * (double)span1;
}

int fs_coverage_all(fs_ctx *ctx, double *out) {
    hipLaunchKernelGGL(fs_k_coverage, dim3(ctx->n_envs), dim3(FS_COV_THREADS), 0, ctx->stream, ctx->d_envs, ctx->d_coverage,
                       0.00625f);
    HIP_TRY(hipGetLastError());
    const size_t bytes = sizeof(double) * ctx->n_envs;
    void *st = fs_stage(ctx, bytes);
    if (!st) return FS_ERR_HIP;
    HIP_TRY(hipMemcpyAsync(st, ctx->d_coverage, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    memcpy(out, st, bytes);
    return FS_OK;
}

// picker meshes of `env` into d_sv / d_sn (float4[441 * shapes]); the shapes' previous rotations are host state
// (pyflex.add_sphere / set_shape_states; the device-side picker moves centres only)
static int launch_sphere_mesh(fs_ctx *ctx, int env, FsVec4 *d_sv, FsVec4 *d_sn) {
    const FsEnv &e = ctx->envs[env];
    static const FsSphereTrig trig = [] { FsSphereTrig t; fs_sphere_trig(t); return t; }();
    FsSphereRot rot;
    memset(&rot, 0, sizeof(rot));
    for (int q = 0; q < e.shapes.count && q < FS_MAX_SHAPES; ++q) fs_quat_axes(e.shape_prev_rot[q], rot.a[q]);
    const size_t sph_verts = size_t(e.shapes.count) * FS_SPHERE_VERTS;
    hipLaunchKernelGGL(fs_k_sphere_mesh, dim3((unsigned)((sph_verts + 255) / 256)), dim3(256), 0, ctx->stream,
                       ctx->d_shapes + env, trig, rot, d_sv, d_sn);
    HIP_TRY(hipGetLastError());
    return FS_OK;
}

// The picker meshes alone (test hook of the render path: what fs_render_device rasterises for the shapes).
// verts4 / nrms4: float[4 * 441 * shapes]; tris: int[3 * 800 * shapes] (either may be null).
int fs_sphere_mesh_env(fs_ctx *ctx, int env, float *verts4, float *nrms4, int *tris) {
    const FsEnv &e = ctx->envs[env];
    const int n_sph = e.shapes.count;
    if (n_sph <= 0) return FS_OK;
    const size_t nv = size_t(n_sph) * FS_SPHERE_VERTS, bytes = nv * 16;
    int rc = ensure_scratch(ctx, 2 * bytes + 512);
    if (rc != FS_OK) return rc;
    FsVec4 *d_sv = (FsVec4 *)ctx->render_scratch, *d_sn = d_sv + nv;
    rc = launch_sphere_mesh(ctx, env, d_sv, d_sn);
    if (rc != FS_OK) return rc;
    char *stg = (char *)fs_stage(ctx, 2 * bytes);
    if (!stg) return FS_ERR_HIP;
    HIP_TRY(hipMemcpyAsync(stg, d_sv, 2 * bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (verts4) memcpy(verts4, stg, bytes);
    if (nrms4) memcpy(nrms4, stg + bytes, bytes);
    if (tris)
        for (int t = 0; t < n_sph * FS_SPHERE_TRIS; ++t) fs_sphere_tri(t, tris[3 * t], tris[3 * t + 1], tris[3 * t + 2]);
    return FS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// pyflex.render -- see fs_raster_kernels.h
// Renders into the context's scratch and leaves the frame there: *d_rgba_out (uint8 RGBA, bottom-up rows) and
// *d_depth_out (float32) stay valid until the next render on this context; the work is enqueued on ctx->stream.
// where one render's passes work: normals | sphere verts | sphere normals | z-buffer (u64 per pixel) | shadow map (u32 per texel)
struct FsRenderScratch {
    FsVec4 *nrm, *sv, *sn;
    unsigned long long *z;
    unsigned int *shadow;
    size_t bytes;  // of the carve (with base = nullptr: how much a render of this shape needs)
};
static FsRenderScratch render_carve(char *base, int n, int n_sph, int W, int H) {
    const size_t sph_verts = size_t(n_sph) * FS_SPHERE_VERTS;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) & ~size_t(255); return o; };
    FsRenderScratch r;
    r.nrm = (FsVec4 *)(base + take(size_t(16) * n));
    r.sv = (FsVec4 *)(base + take(size_t(16) * (sph_verts + 1)));
    r.sn = (FsVec4 *)(base + take(size_t(16) * (sph_verts + 1)));
    r.z = (unsigned long long *)(base + take(size_t(8) * W * H));
    r.shadow = (unsigned int *)(base + take(size_t(4) * FS_SHADOW_RES * FS_SHADOW_RES));
    r.bytes = off;
    return r;
}
// The passes of one frame of `env` at W x H on ctx->stream, shared by both forms of the renderer so that they cannot drift
// apart: normals, cleared z-buffer and shadow map, picker meshes (from the DEVICE shape states), shadow pass (depth only, from
// the light), camera pass (depth + primitive id), shading.  d_depth != nullptr: pyflex.render's outputs (RGBA8 bottom-up into
// d_color + linear depth); nullptr: the capture form (RGB8 top-down into d_color).
static int launch_render_passes(fs_ctx *ctx, int env, int W, int H, const FsRenderScratch &sc, unsigned char *d_color, float *d_depth) {
    FsEnv &e = ctx->envs[env];
    const int T = e.host.t, n_sph = e.shapes.count;
    FsRasterFrame fr;
    fs_raster_setup(fr, e.cam.pos, e.cam.angle, W, H, e.host.scene_lower, e.host.scene_upper);
    hipStream_t st = ctx->stream;
    int rc = launch_normals(ctx, e, sc.nrm);
    if (rc != FS_OK) return rc;
    HIP_TRY(hipMemsetAsync(sc.z, 0xff, size_t(8) * W * H, st));
    HIP_TRY(hipMemsetAsync(sc.shadow, 0xff, size_t(4) * FS_SHADOW_RES * FS_SHADOW_RES, st));
    if (n_sph > 0) {
        rc = launch_sphere_mesh(ctx, env, sc.sv, sc.sn);
        if (rc != FS_OK) return rc;
    }
    const int n_sph_tris = n_sph * FS_SPHERE_TRIS, total_tris = T + n_sph_tris;
    if (total_tris > 0) {
        hipLaunchKernelGGL(fs_k_raster_shadow, dim3((total_tris + 63) / 64), dim3(64), 0, st, fr, e.dev.pos, e.topo->tris, T,
                           sc.sv, n_sph_tris, sc.shadow);
        hipLaunchKernelGGL(fs_k_raster_camera, dim3((total_tris + 63) / 64), dim3(64), 0, st, fr, e.dev.pos, e.topo->tris, T,
                           sc.sv, n_sph_tris, sc.z);
    }
    // the episode's appearance (fs_set_appearance): the colours ride in the frame, which the shader is linear in before the
    // gamma; only a textured ground needs kernels of its own
    const fs_appearance &look = e.look;
    for (int k = 0; k < 3; ++k) { fr.col_cloth[k] = look.cloth_rgb[k]; fr.col_plane[k] = look.ground_rgb[0][k]; }
    const dim3 grid((W + 15) / 16, (H + 15) / 16), block(16, 16);
    if (look.ground_octaves > 0) {
        if (d_depth)
            hipLaunchKernelGGL(fs_k_shade_tex, grid, block, 0, st, fr, e.dev.pos, sc.nrm, e.topo->tris, T, sc.sv, sc.sn, n_sph_tris,
                               sc.z, sc.shadow, d_color, d_depth, look);
        else
            hipLaunchKernelGGL(fs_k_shade_capture_tex, grid, block, 0, st, fr, e.dev.pos, sc.nrm, e.topo->tris, T, sc.sv, sc.sn,
                               n_sph_tris, sc.z, sc.shadow, d_color, look);
    } else if (d_depth)
        hipLaunchKernelGGL(fs_k_shade, grid, block, 0, st, fr, e.dev.pos, sc.nrm, e.topo->tris, T, sc.sv, sc.sn, n_sph_tris, sc.z,
                           sc.shadow, d_color, d_depth);
    else
        hipLaunchKernelGGL(fs_k_shade_capture, grid, block, 0, st, fr, e.dev.pos, sc.nrm, e.topo->tris, T, sc.sv, sc.sn,
                           n_sph_tris, sc.z, sc.shadow, d_color);
    HIP_TRY(hipGetLastError());
    return FS_OK;
}

int fs_render_device(fs_ctx *ctx, int env, unsigned char **d_rgba_out, float **d_depth_out) {
    FsEnv &e = ctx->envs[env];
    const int W = e.cam.width, H = e.cam.height;
    if (W <= 0 || H <= 0 || W > 4096 || H > 4096) { fs_set_error("bad camera size"); return FS_ERR_ARG; }
    // the context's scratch: the passes' carve | rgba | depth
    const size_t o_rgba = render_carve(nullptr, e.host.n, e.shapes.count, W, H).bytes;
    const size_t o_depth = o_rgba + ((size_t(4) * W * H + 255) & ~size_t(255));
    int rc = ensure_scratch(ctx, o_depth + ((size_t(4) * W * H + 255) & ~size_t(255)));
    if (rc != FS_OK) return rc;
    char *base = (char *)ctx->render_scratch;
    unsigned char *d_rgba = (unsigned char *)(base + o_rgba);
    float *d_depth = (float *)(base + o_depth);
    rc = launch_render_passes(ctx, env, W, H, render_carve(base, e.host.n, e.shapes.count, W, H), d_rgba, d_depth);
    if (rc != FS_OK) return rc;
    *d_rgba_out = d_rgba;
    *d_depth_out = d_depth;
    return FS_OK;
}

int fs_render_env(fs_ctx *ctx, int env, unsigned char *rgba, float *depth) {
    unsigned char *d_rgba = nullptr;
    float *d_depth = nullptr;
    int rc = fs_render_device(ctx, env, &d_rgba, &d_depth);
    if (rc != FS_OK) return rc;
    const FsEnv &e = ctx->envs[env];
    hipStream_t st = ctx->stream;
    const size_t px = size_t(e.cam.width) * e.cam.height;
    char *stg = (char *)fs_stage(ctx, px * 8);
    if (!stg) return FS_ERR_HIP;
    HIP_TRY(hipMemcpyAsync(stg, d_rgba, px * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(stg + px * 4, d_depth, px * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    memcpy(rgba, stg, px * 4);
    memcpy(depth, stg + px * 4, px * 4);
    return FS_OK;
}

// The intermediate buffers of one fs_render_device frame of `env` (test hook of the render path): the z-buffer plane the
// camera pass left (depth24 << 32 | primitive id per pixel, all ones where no triangle landed; the ground plane joins in the
// shading pass and is not in it) and the 2048^2 shadow map (depth24 per texel, all ones where cleared).  Either may be null.
int fs_render_buffers_env(fs_ctx *ctx, int env, unsigned long long *zkeys, unsigned int *shadow) {
    unsigned char *d_rgba = nullptr;
    float *d_depth = nullptr;
    int rc = fs_render_device(ctx, env, &d_rgba, &d_depth);
    if (rc != FS_OK) return rc;
    const FsEnv &e = ctx->envs[env];
    const int W = e.cam.width, H = e.cam.height;
    const FsRenderScratch sc = render_carve((char *)ctx->render_scratch, e.host.n, e.shapes.count, W, H);  // (as fs_render_device carved it)
    hipStream_t st = ctx->stream;
    if (zkeys) HIP_TRY(hipMemcpyAsync(zkeys, sc.z, size_t(8) * W * H, hipMemcpyDeviceToHost, st));
    if (shadow) HIP_TRY(hipMemcpyAsync(shadow, sc.shadow, size_t(4) * FS_SHADOW_RES * FS_SHADOW_RES, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return FS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Frame capture during movep (SimEnv.movep with dump_visualizations, simEnv.py:764-768: env_video_frames['top'] gets
// get_image()[0] after every fourth loop iteration).  The frames are taken on the device, inside the launch sequences of
// fs_movep_batch / fs_advance_begin (fs_picker.hip), so the capture form of the renderer
//   - writes RGB8, rows top-down, straight into a slot of the call's frame store (fs_k_shade_capture): no depth plane, no
//     RGBA intermediate, no staging copy, no synchronise;
//   - carves its scratch out of a buffer the EPISODE owns (FsEnv::cap_scratch), taken from the pool when capture is switched
//     on: the context's render_scratch may be reallocated, and the observation stage uses it on the service lane while a
//     chunk with captures is in flight on the main stream;
//   - reads the picker spheres from the device (ctx->d_shapes, as launch_sphere_mesh does): the host mirror already holds
//     the END of a planned trajectory when the launches are queued;
//   - renders at its own width and height with the episode's camera pose (projection from fs_raster_setup).
int fs_capture_render(fs_ctx *ctx, int env, unsigned char *d_rgb) {
    FsEnv &e = ctx->envs[env];
    // the scratch is sized for FS_MAX_SHAPES spheres and cap_n particles (fs_set_scene switches capture off, so a scene
    // cannot outgrow it; checked all the same: a render must never write past its carve)
    const FsRenderScratch sc = render_carve((char *)e.cap_scratch, e.cap_n, FS_MAX_SHAPES, e.cap_w, e.cap_h);
    if (!e.cap_on || !e.cap_scratch || e.host.n > e.cap_n || sc.bytes > e.cap_scratch_bytes) {
        fs_set_error("capture: the episode has no capture scratch for its scene (fs_capture_enable after fs_set_scene)");
        return FS_ERR_STATE;
    }
    return launch_render_passes(ctx, env, e.cap_w, e.cap_h, sc, d_rgb, nullptr);
}

void fs_capture_off(fs_ctx *ctx, FsEnv &e) {
    if (e.cap_scratch) fs_pool_give(ctx, e.cap_scratch, e.cap_scratch_bytes);  // (its renders have completed: callers make sure)
    e.cap_scratch = nullptr; e.cap_scratch_bytes = 0;
    e.cap_on = false;
}

static FsEnv *capture_env(fs_ctx *ctx, int env) {
    if (!ctx || env < 0 || env >= ctx->n_envs) { fs_set_error("capture: bad env"); return nullptr; }
    return &ctx->envs[env];
}
// an open ticket (or none) still renders into / reads the episode's capture state
static bool capture_in_flight(const fs_ctx *ctx, int env) {
    for (const FsAdvTicket &t : ctx->tickets) {
        if (!t.busy) continue;
        for (const FsCapSlot &s : t.cap.slots)
            if (s.env == env) return true;
    }
    return false;
}

extern "C" int fs_capture_enable(fs_ctx *ctx, int env, int width, int height) {
    FsEnv *e = capture_env(ctx, env);
    if (!e) return FS_ERR_ARG;
    if (!e->has_scene) { fs_set_error("fs_capture_enable: the episode has no scene"); return FS_ERR_STATE; }
    if (width <= 0 || height <= 0 || width > 4096 || height > 4096) { fs_set_error("fs_capture_enable: bad frame size"); return FS_ERR_ARG; }
    // host-side checks first, before any HIP call: an episode a chunk in flight moves (or films) keeps its capture state
    if (const int guard_rc = fs_lane_guard(ctx, env)) return guard_rc;
    if (capture_in_flight(ctx, env)) { fs_set_error("fs_capture_enable: a chunk in flight films this episode (fs_advance_end first)"); return FS_ERR_STATE; }
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t need = render_carve(nullptr, e->host.n, FS_MAX_SHAPES, width, height).bytes;
    if (need > e->cap_scratch_bytes) {
        if (e->cap_scratch) fs_pool_give(ctx, e->cap_scratch, e->cap_scratch_bytes);
        e->cap_scratch_bytes = 0;
        e->cap_scratch = fs_pool_take(ctx, need, &e->cap_scratch_bytes);
        if (!e->cap_scratch) { e->cap_on = false; return FS_ERR_HIP; }
    }
    if (e->cap_w != width || e->cap_h != height) e->cap_frames.clear();  // frames of another size cannot be mixed, capture on or off
    e->cap_on = true;
    e->cap_w = width; e->cap_h = height; e->cap_n = e->host.n;
    return FS_OK;
}

extern "C" int fs_capture_disable(fs_ctx *ctx, int env) {
    FsEnv *e = capture_env(ctx, env);
    if (!e) return FS_ERR_ARG;
    if (const int guard_rc = fs_lane_guard(ctx, env)) return guard_rc;
    if (capture_in_flight(ctx, env)) { fs_set_error("fs_capture_disable: a chunk in flight films this episode (fs_advance_end first)"); return FS_ERR_STATE; }
    fs_capture_off(ctx, *e);  // (its renders have completed: no ticket films it)
    return FS_OK;  // frames not yet taken stay until fs_capture_take
}

extern "C" int fs_capture_count(const fs_ctx *ctx, int env) {
    if (!ctx || env < 0 || env >= ctx->n_envs) return FS_ERR_ARG;
    const FsEnv &e = ctx->envs[env];
    const size_t frame = size_t(3) * e.cap_w * e.cap_h;
    return frame ? (int)(e.cap_frames.size() / frame) : 0;
}

extern "C" int fs_capture_size(const fs_ctx *ctx, int env, int *width, int *height) {
    if (!ctx || env < 0 || env >= ctx->n_envs || !width || !height) return FS_ERR_ARG;
    *width = ctx->envs[env].cap_w; *height = ctx->envs[env].cap_h;
    return ctx->envs[env].cap_on ? 1 : 0;
}

extern "C" int fs_capture_take(fs_ctx *ctx, int env, unsigned char *out, long long n_bytes) {
    FsEnv *e = capture_env(ctx, env);
    if (!e) return FS_ERR_ARG;
    const int frames = fs_capture_count(ctx, env);
    if (frames > 0) {
        if (!out || n_bytes < (long long)e->cap_frames.size()) { fs_set_error("fs_capture_take: buffer too small"); return FS_ERR_ARG; }
        memcpy(out, e->cap_frames.data(), e->cap_frames.size());
    }
    std::vector<unsigned char>().swap(e->cap_frames);  // handed over and forgotten
    return frames;
}

// ---------------------------------------------------------------------------------------------------------------
// Per-episode appearance (include/flingsim.h): host state of FsEnv, read by launch_render_passes when a render is queued.
extern "C" int fs_appearance_default(fs_appearance *out) {
    if (out) *out = fs_default_appearance();
    return (int)sizeof(fs_appearance);
}

// the texture rule on the host (the function the shading kernels inline, compiled for the CPU): t[k] at (hx[k], hz[k])
extern "C" int fs_host_ground_texture(const fs_appearance *a, int n, const float *hx, const float *hz, float *t) {
    if (n < 0 || (n > 0 && (!hx || !hz || !t))) { fs_set_error("fs_host_ground_texture: bad arguments"); return FS_ERR_ARG; }
    if (const int rc = fs_appearance_check(a)) return rc;
    for (int k = 0; k < n; ++k) t[k] = fs_ground_noise(a->ground_seed, a->ground_cells_per_m, a->ground_octaves, hx[k], hz[k]);
    return FS_OK;
}

extern "C" int fs_appearance_check(const fs_appearance *a) {
    if (!a) { fs_set_error("fs_appearance: null appearance"); return FS_ERR_ARG; }
    const float *alb[3] = {a->cloth_rgb, a->ground_rgb[0], a->ground_rgb[1]};
    for (int q = 0; q < 3; ++q)
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(alb[q][k]) || alb[q][k] < 0.0f) { fs_set_error("fs_appearance: an albedo is negative or not finite"); return FS_ERR_ARG; }
    if (a->ground_octaves < 0 || a->ground_octaves > 6) { fs_set_error("fs_appearance: ground_octaves outside 0 .. 6"); return FS_ERR_ARG; }
    if (a->ground_octaves > 0) {
        const float c = a->ground_cells_per_m;
        if (!std::isfinite(c) || c <= 0.0f) { fs_set_error("fs_appearance: ground_cells_per_m must be positive"); return FS_ERR_ARG; }
        if (c * (float)(1 << (a->ground_octaves - 1)) > 256.0f) {
            fs_set_error("fs_appearance: the finest octave exceeds 256 cells per metre (the texture is not filtered)");
            return FS_ERR_ARG;
        }
    }
    return FS_OK;
}

extern "C" int fs_set_appearance(fs_ctx *ctx, int n, const int *envs, const fs_appearance *table) {
    if (!ctx || n < 1 || !envs || !table) { fs_set_error("fs_set_appearance: bad arguments"); return FS_ERR_ARG; }
    // every refusal before anything changes
    for (int k = 0; k < n; ++k) {
        if (envs[k] < 0 || envs[k] >= ctx->n_envs) { fs_set_error("fs_set_appearance: env index out of range"); return FS_ERR_ARG; }
        if (!ctx->envs[envs[k]].has_scene) { fs_set_error("fs_set_appearance: the episode has no scene"); return FS_ERR_ARG; }
        if (const int rc = fs_appearance_check(table + k)) return rc;
    }
    for (int k = 0; k < n; ++k)
        if (capture_in_flight(ctx, envs[k])) {
            fs_set_error("fs_set_appearance: a chunk in flight films this episode (fs_advance_end first)");
            return FS_ERR_STATE;
        }
    for (int k = 0; k < n; ++k) ctx->envs[envs[k]].look = table[k];
    return FS_OK;
}

extern "C" int fs_get_appearance(fs_ctx *ctx, int env, fs_appearance *out) {
    FsEnv *e = capture_env(ctx, env);
    if (!e || !out) { if (e) fs_set_error("fs_get_appearance: null output"); return FS_ERR_ARG; }
    *out = e->has_scene ? e->look : fs_default_appearance();
    return FS_OK;
}
