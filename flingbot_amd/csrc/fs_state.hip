// fs_state.hip -- particle state as batched device tensors (additive: the reference hands particle arrays over one episode at
// a time through host memory, pyflex.cpp get_positions / set_positions and their kin).  fs_state_gather packs the positions,
// velocities and phases of a list of episodes into padded [n, n_max] device arrays, fs_state_scatter writes such arrays back:
// one launch per call for every listed episode and every requested field.  Both are pure copies in the 16-byte elements the
// slabs already hold (pos float4[N], vel float4[N]): a lane moves one particle's float4 with one dwordx4 load and one dwordx4
// store, the 64 lanes of a wave cover 1 KiB of consecutive addresses on both sides.  The kernels find the slabs through the
// FsEnvDev descriptors that are on the device already; only the episode list goes up.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/flingsim.h"
#include "fs_context.h"

#define HIP_TRY(call)                                     \
    do {                                                  \
        if (!fs_hip_ok((call), #call)) return FS_ERR_HIP; \
    } while (0)

#define FS_STATE_TILE 256  // particles per workgroup

// Workgroup b serves (row b / tiles, tile b % tiles) of the padded batch.  Every tile of a gather has bytes to write -- state
// below the row's count, zeros from there to n_max -- so none idles; a tile that straddles the count does both.
__global__ __launch_bounds__(FS_STATE_TILE) void fs_k_state_gather(const FsEnvDev *__restrict__ envs, const int *__restrict__ ids,
                                                                   int n_max, int tiles, uint4 *__restrict__ pos4,
                                                                   uint4 *__restrict__ vel4, int *__restrict__ phase) {
    const int row = blockIdx.x / tiles, tile = blockIdx.x - row * tiles;
    const int i = tile * FS_STATE_TILE + threadIdx.x;
    if (i >= n_max) return;
    const FsEnvDev &E = envs[ids[row]];
    const bool live = i < E.n;
    const size_t o = (size_t)row * n_max + i;
    if (pos4) {
        uint4 v = uint4{0u, 0u, 0u, 0u};
        if (live) v = ((const uint4 *)E.pos)[i];
        pos4[o] = v;
    }
    if (vel4) {
        uint4 v = uint4{0u, 0u, 0u, 0u};
        if (live) v = ((const uint4 *)E.vel)[i];
        vel4[o] = v;
    }
    if (phase) {  // (4 bytes a lane: a row of n_max ints need not start on 16 bytes)
        int v = 0;
        if (live) v = E.phase[i];
        phase[o] = v;
    }
}

// The same indexing; a tile at or beyond the row's count ends after two scalar loads (its rows are never read), so a short
// row of a mixed-size launch costs no memory traffic.  The fourth velocity lane is stored as 0, as fs_set_velocities does.
__global__ __launch_bounds__(FS_STATE_TILE) void fs_k_state_scatter(const FsEnvDev *__restrict__ envs, const int *__restrict__ ids,
                                                                    int n_max, int tiles, const uint4 *__restrict__ pos4,
                                                                    const uint4 *__restrict__ vel4) {
    const int row = blockIdx.x / tiles, tile = blockIdx.x - row * tiles;
    const FsEnvDev &E = envs[ids[row]];
    if (tile * FS_STATE_TILE >= E.n) return;
    const int i = tile * FS_STATE_TILE + threadIdx.x;
    if (i >= E.n) return;
    const size_t o = (size_t)row * n_max + i;
    if (pos4) ((uint4 *)E.pos)[i] = pos4[o];
    if (vel4) {
        uint4 v = vel4[o];
        v.w = 0u;
        ((uint4 *)E.vel)[i] = v;
    }
}

// The argument rules both calls share; nothing is touched before the whole list has passed.
static int state_check(const fs_ctx *ctx, const char *who, int n, const int *envs, int n_max) {
    const std::string w(who);
    for (int k = 0; k < n; ++k) {
        const int e = envs[k];
        if (e < 0 || e >= ctx->n_envs) { fs_set_error(w + ": env index " + std::to_string(e) + " out of range"); return FS_ERR_ARG; }
        if (!ctx->envs[e].has_scene) { fs_set_error(w + ": episode " + std::to_string(e) + " has no scene"); return FS_ERR_ARG; }
    }
    for (int k = 0; k < n; ++k)
        if (ctx->envs[envs[k]].host.n > n_max) {
            fs_set_error(w + ": n_max " + std::to_string(n_max) + " is below the " + std::to_string(ctx->envs[envs[k]].host.n) +
                         " particles of episode " + std::to_string(envs[k]));
            return FS_ERR_ARG;
        }
    const long long blocks = (long long)n * ((n_max + FS_STATE_TILE - 1) / FS_STATE_TILE);
    if (blocks > 0x7fffffffLL) { fs_set_error(w + ": n x n_max is beyond one launch"); return FS_ERR_ARG; }
    return FS_OK;
}

// The list goes up the way fs_fork's table does: written into a pinned image, copied by the stream in front of the launch.
static int state_upload(fs_ctx *ctx, int n, const int *envs) {
    if ((size_t)n > ctx->state_cap) {
        fs_sync_all_streams(ctx);
        if (ctx->state_d) (void)hipFree(ctx->state_d);
        if (ctx->state_h) (void)hipHostFree(ctx->state_h);
        ctx->state_d = ctx->state_h = nullptr;
        ctx->state_cap = 0;
        const size_t cap = (size_t)n * 2 < 1024 ? 1024 : (size_t)n * 2;
        HIP_TRY(hipHostMalloc((void **)&ctx->state_h, sizeof(int) * cap, hipHostMallocDefault));
        HIP_TRY(hipMalloc((void **)&ctx->state_d, sizeof(int) * cap));
        ctx->state_cap = cap;
    }
    for (int k = 0; k < n; ++k) ctx->state_h[k] = envs[k];
    HIP_TRY(hipMemcpyAsync(ctx->state_d, ctx->state_h, sizeof(int) * n, hipMemcpyHostToDevice, ctx->stream));
    return FS_OK;
}

extern "C" int fs_state_gather(fs_ctx *ctx, int n, const int *envs, int n_max, float *d_pos4, float *d_vel4, int *d_phase,
                               int *counts) {
    if (!ctx || !envs || n <= 0 || n_max <= 0) { fs_set_error("fs_state_gather: null context / null list / n < 1 / n_max < 1"); return FS_ERR_ARG; }
    if (!d_pos4 && !d_vel4 && !d_phase) { fs_set_error("fs_state_gather: no field asked for (d_pos4, d_vel4 and d_phase are all null)"); return FS_ERR_ARG; }
    if (fs_misaligned16({d_pos4, d_vel4}) || ((uintptr_t)d_phase & 3)) { fs_set_error("fs_state_gather: d_pos4 / d_vel4 off a 16-byte boundary"); return FS_ERR_ARG; }
    int rc = state_check(ctx, "fs_state_gather", n, envs, n_max);
    if (rc != FS_OK) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    rc = state_upload(ctx, n, envs);
    if (rc != FS_OK) return rc;
    const int tiles = (n_max + FS_STATE_TILE - 1) / FS_STATE_TILE;
    hipLaunchKernelGGL(fs_k_state_gather, dim3((unsigned)n * (unsigned)tiles), dim3(FS_STATE_TILE), 0, ctx->stream, ctx->d_envs,
                       (const int *)ctx->state_d, n_max, tiles, (uint4 *)d_pos4, (uint4 *)d_vel4, d_phase);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // the tensors are the caller's from here on, on any stream
    if (counts)
        for (int k = 0; k < n; ++k) counts[k] = ctx->envs[envs[k]].host.n;
    return FS_OK;
}

extern "C" int fs_state_scatter(fs_ctx *ctx, int n, const int *envs, int n_max, const float *d_pos4, const float *d_vel4) {
    if (!ctx || !envs || n <= 0 || n_max <= 0) { fs_set_error("fs_state_scatter: null context / null list / n < 1 / n_max < 1"); return FS_ERR_ARG; }
    if (!d_pos4 && !d_vel4) { fs_set_error("fs_state_scatter: no field given (d_pos4 and d_vel4 are both null)"); return FS_ERR_ARG; }
    if (fs_misaligned16({d_pos4, d_vel4})) { fs_set_error("fs_state_scatter: d_pos4 / d_vel4 off a 16-byte boundary"); return FS_ERR_ARG; }
    int rc = state_check(ctx, "fs_state_scatter", n, envs, n_max);
    if (rc != FS_OK) return rc;
    std::vector<char> listed((size_t)ctx->n_envs, 0);
    for (int k = 0; k < n; ++k) {
        if (listed[envs[k]]) { fs_set_error("fs_state_scatter: destination " + std::to_string(envs[k]) + " is listed twice"); return FS_ERR_ARG; }
        listed[envs[k]] = 1;
    }
    for (int k = 0; k < n; ++k)
        if (const int guard_rc = fs_lane_guard(ctx, envs[k])) return guard_rc;
    HIP_TRY(hipSetDevice(ctx->device));
    rc = state_upload(ctx, n, envs);
    if (rc != FS_OK) return rc;
    const int tiles = (n_max + FS_STATE_TILE - 1) / FS_STATE_TILE;
    hipLaunchKernelGGL(fs_k_state_scatter, dim3((unsigned)n * (unsigned)tiles), dim3(FS_STATE_TILE), 0, ctx->stream, ctx->d_envs,
                       (const int *)ctx->state_d, n_max, tiles, (const uint4 *)d_pos4, (const uint4 *)d_vel4);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // the caller may rewrite its tensors as soon as the call returns
    return FS_OK;
}
