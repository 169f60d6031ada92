/*
 * flingsim.h -- C-ABI of the MI355X-native FlingBot cloth hot path (libflingsim.so).
 *
 * This is the drop-in boundary: every entry point replaces one function of the reference's `pyflex` pybind11
 * module (PyFlex/bindings/pyflex.cpp, cited per function) and takes only plain pointers and sizes, so the
 * reference's own binding layer (pybind11), ctypes, cffi or any other FFI can bind it (INTEGRATION.md shows the stubs).
 *
 * Differences from the reference boundary, all additive:
 *   - the reference is a process-global singleton (one g_solver, main.cpp:163); here a context owns `n_envs`
 *     independent cloth episodes that step in ONE batched launch.  `pyflex.*` == env 0 of a 1-env context.
 *   - errors are return codes (0 = ok, <0 = error) + fs_last_error(), instead of printf/exit (pyflex.cpp:103-107).
 *   - the caller owns every host buffer; `n_*` arguments are ELEMENT counts (floats / ints), and are checked.
 *
 * There is no CPU fallback: fs_create fails if no HIP device is usable.
 */
#ifndef FLINGSIM_H
#define FLINGSIM_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fs_ctx fs_ctx;

#define FS_OK 0
#define FS_ERR_ARG (-1)
#define FS_ERR_HIP (-2)
#define FS_ERR_STATE (-3)
#define FS_ERR_LIMIT (-4) /* fs_movep: step limit reached (MoveJointsException, environment/exceptions.py) */

/* solver back-ends (fs_set_solver) */
#define FS_SOLVER_AUTO 0    /* fused LDS-resident kernel when the episode fits one CU's LDS, else streaming */
#define FS_SOLVER_STREAM 1  /* per-stage kernels over HBM-resident SoA state (any particle count) */
#define FS_SOLVER_FUSED 2   /* one workgroup per episode, particle state resident in LDS for the whole step */
#define FS_SOLVER_FUSED_GENERIC 3 /* FUSED, but spring adjacency streamed from L2 instead of register-resident */
#define FS_SOLVER_STREAM_ELL 4    /* STREAM, but with the uncompressed (index, length, stiffness) adjacency arrays */
#define FS_SOLVER_FUSED_CODED 5   /* FUSED, but never the grid-64 form: the dictionary-coded adjacency kernel */
#define FS_SOLVER_STREAM_CODED 6  /* STREAM, but never the grid-L form: coded / latency / grid forms chosen by launch size */
#define FS_SOLVER_STREAM_SPLIT 7  /* STREAM, but the substep boundary as separate finalize / predict / scan / scatter launches
                                     (the form cloths above 16384 particles and launches of fewer than 16 episodes take)
                                     instead of fs_k_boundary */
#define FS_SOLVER_STREAM_MERGED 8 /* STREAM, with fs_k_boundary at every launch size */
#define FS_SOLVER_COTENANT 9      /* for a process that SHARES the device with others (fs_tenants_*): every launch whose episodes
                                     all fit the fused kernel takes it whatever the launch size (one launch per frame on one
                                     compute unit each -- co-tenants' frames run side by side), every other launch is AUTO's */
#define FS_SOLVER_STREAM_MESH 10  /* STREAM, with the per-episode iterate forms at EVERY launch size (also below the latency
                                     threshold): a launch in which some cloth has no stream codes runs fs_k_iterate_mesh when
                                     every cloth has packed mesh words, fs_k_iterate_mixed when the episodes' forms differ
                                     (fs_last_slot_forms).  The tests use it to reach these kernels at small shapes. */
/* The iterate kernel of a streaming launch.  FS_SOLVER_STREAM (1) picks ONE kernel for the whole launch list from what every
   episode allows, exactly as before the per-episode forms existed: one cloth without stream codes puts the launch on
   fs_k_iterate<false> (FS_FORM_STREAM_ELL).  It is the comparison id of scripts/shirt_eval_timing.py and stays that way.
   FS_SOLVER_STREAM_MESH applies the per-episode rule at every size.  FS_SOLVER_AUTO (and FS_SOLVER_COTENANT where it defers
   to AUTO) applies it to launches above the latency threshold (32 x 4096 particles) for the launch classes that have passed
   their measurement (EXPERIMENTS R29.1; both have): FS_AUTO_MESH_KERNEL / FS_AUTO_MIXED_KERNEL in fs_solver.hip.  The rule only ever
   replaces fs_k_iterate<false> (and, under id 10, the latency form of such a launch): a launch whose cloths all have stream
   codes keeps its kernel.  Per slot: gp_L_ok && gp_halvable -> the grid-L throughput body; else stream codes -> the coded
   body; else mesh words -> the mesh body; else the ELL body.  Results are bit-identical in every form. */

const char *fs_last_error(void);
int fs_version(void);

/* pyflex.init (pyflex.cpp:15-124): create the solver/renderer context on HIP device `device` for `n_envs` episodes.
   camera_width/height are the render target size (g_screenWidth/Height). */
fs_ctx *fs_create(int device, int n_envs, int camera_width, int camera_height);
/* pyflex.clean (pyflex.cpp:126-160) */
void fs_destroy(fs_ctx *ctx);
int fs_n_envs(const fs_ctx *ctx);
int fs_set_solver(fs_ctx *ctx, int solver);
int fs_get_solver(const fs_ctx *ctx);
/* 1 when FS_SOLVER_FUSED can step this episode (<= 4096 particles, one collision plane at most), 0 when it cannot (the
   caller then keeps FS_SOLVER_AUTO): lets a front end choose the back-end when a scene is set instead of finding out from a
   failed fs_step */
int fs_fused_fits(fs_ctx *ctx, int env);

/* Co-tenant table (csrc/fs_tenants.cpp): the reference runs one PyFleX per Ray worker on one GPU (`--num_processes 16`,
   README.md:147-148, utils.py:144-157); the processes of one user that drive the same physical device through this library find
   each other in a small mmap-ed file per (user, device) under /dev/shm (FLINGSIM_TENANT_DIR overrides), so that the `pyflex`
   module can pick FS_SOLVER_COTENANT by itself.  `device_key` names the physical device: fs_device_key() = its PCI bus id.
   fs_tenants_register: add this process, returns the number of live tenants including it; fs_tenants_count: live tenants
   (prune > 0: also clear the entries of processes that died without unregistering; prune < 0: the number of occupied slots as
   they stand, no liveness check, no system call); fs_tenants_unregister: remove this process.
   Host-only (no HIP call): usable, and tested, without a GPU. */
int fs_device_key(fs_ctx *ctx, char *out, int n_chars);
int fs_tenants_register(const char *device_key);
int fs_tenants_count(const char *device_key, int prune);
int fs_tenants_unregister(const char *device_key);

/* pyflex.set_scene (pyflex.cpp:229-244 -> main.cpp:613 Init -> softgym_cloth.h:33 Initialize).
   scene_params[19] layout: flex_utils.py:332-342.  Empty `verts` selects the grid path (helpers.h:838). */
int fs_set_scene(fs_ctx *ctx, int env, const float *scene_params, int n_params, const float *verts, int n_vert_floats,
                 const int *stretch, int n_stretch_ints, const int *bend, int n_bend_ints, const int *shear,
                 int n_shear_ints, const int *faces, int n_face_ints);

/* pyflex.step (pyflex.cpp:213-222 -> main.cpp:2120 UpdateFrame -> NvFlexUpdateSolver(dt, substeps)).
   Advances env (or every env with a scene when env == -1) by n_steps frames.  Asynchronous on the context's HIP
   stream; every getter synchronises. */
int fs_step(fs_ctx *ctx, int env, int n_steps);
/* the same for a list of episodes (each listed once): one batched launch sequence for exactly those */
int fs_step_list(fs_ctx *ctx, int n, const int *envs, int n_steps);
int fs_sync(fs_ctx *ctx);
/* fs_step bracketed by HIP events recorded on the context's stream; returns the elapsed device time of the launch(es)
   in milliseconds.  Used by bench.py for the per-launch kernel duration (roofline). */
int fs_step_timed(fs_ctx *ctx, int env, int n_steps, float *elapsed_ms);
/* HIP-event stopwatch on the context's stream (non-blocking start; stop waits for the stream to reach it). */
int fs_timer_start(fs_ctx *ctx);
int fs_timer_stop(fs_ctx *ctx, float *elapsed_ms);
/* the HIP stream (hipStream_t) the context launches on, for callers that time with HIP events */
void *fs_stream(fs_ctx *ctx);

/* counts: pyflex.get_n_particles :326, get_n_shapes :334; springs / triangles implied by get_edges / get_faces */
int fs_n_particles(const fs_ctx *ctx, int env);
int fs_n_springs(const fs_ctx *ctx, int env);
int fs_n_triangles(const fs_ctx *ctx, int env);
int fs_n_shapes(const fs_ctx *ctx, int env);

/* particle mirrors.  get_positions :414 / set_positions :464 (float[4N] xyz + invMass),
   get_velocities :753 / set_velocities :772 (float[3N]), get_phases :378 / set_phases :395 (int[N]),
   get_restPositions (float[4N]), get_edges :433 (int[2M]), get_faces :449 (int[3T]). */
int fs_get_positions(fs_ctx *ctx, int env, float *out, int n_floats);
int fs_set_positions(fs_ctx *ctx, int env, const float *in, int n_floats);
int fs_get_velocities(fs_ctx *ctx, int env, float *out, int n_floats);
int fs_set_velocities(fs_ctx *ctx, int env, const float *in, int n_floats);
int fs_get_phases(fs_ctx *ctx, int env, int *out, int n_ints);
int fs_set_phases(fs_ctx *ctx, int env, const int *in, int n_ints);
int fs_get_rest_positions(fs_ctx *ctx, int env, float *out, int n_floats);
int fs_get_normals(fs_ctx *ctx, int env, float *out, int n_floats); /* NvFlexGetNormals, main.cpp:2286 */
int fs_get_edges(fs_ctx *ctx, int env, int *out, int n_ints);
int fs_get_faces(fs_ctx *ctx, int env, int *out, int n_ints);
int fs_get_spring_lengths(fs_ctx *ctx, int env, float *out, int n_floats);
int fs_get_spring_stiffness(fs_ctx *ctx, int env, float *out, int n_floats);
/* effective NvFlexParams of the env as a packed float[32] (layout: DESIGN.md "parameter table") */
int fs_get_params(fs_ctx *ctx, int env, float *out, int n_floats);
/* overwrite the packed parameter table (same layout as fs_get_params); used for experiments and by the parameter-sweep
   tests -- FlingBot never changes the solver parameters after set_scene.  Per episode; takes effect at the next launch
   (the descriptor is rewritten, which also rebuilds the streaming back-end's cached launch table); fs_set_scene restores
   the defaults, fs_fork carries the table to its destination.  Slot by slot:
     APPLIED   0 numIterations (0..1000, truncated), 1 numSubsteps (1..100, truncated), 2 dt (> 0), 3-5 gravity,
               7 solidRestDistance, 8 collisionDistance, 9 shapeCollisionMargin, 11 dynamicFriction, 12 staticFriction,
               13 particleFriction, 14 damping, 15 sleepThreshold, 16 relaxationFactor, 17 maxAcceleration, 18 maxSpeed,
               23-26 planes[0], 27 maxNeighbors (an integer in 1..96), 28 maxContacts (an integer in 0..24: the candidate
               mask of collideShapes has 8 plane bits + 16 sphere bits)
     REFUSED   when different from the current value: 6 radius and 10 particleCollisionMargin (baked into the topology's
               rest-pose filter), 22 numPlanes (planes[0] only), 29 relaxationMode (local relaxation only)
     IGNORED   19-21 restitution / adhesion / dissipation (nothing reads them; fs_get_params keeps reporting the scene's),
               30-31 (unused)
   A value outside its range, a refused slot or a table shorter than 32 returns FS_ERR_ARG and changes nothing.  Episodes
   stepped together must share numSubsteps and numIterations, and the streaming back-end steps at most 8 substeps per frame
   (FS_ERR_STATE from fs_step otherwise, nothing launched); the fused kernels index nothing by substep and take any count. */
int fs_set_params(fs_ctx *ctx, int env, const float *in, int n_floats);
/* pyflex.get_scene_lower / get_scene_upper (pyflex.cpp:865-889) */
int fs_get_scene_bounds(fs_ctx *ctx, int env, float *lower3, float *upper3);

/* shapes.  add_sphere :311 (helpers.h:484), clear_shapes (helpers.h:1677),
   get_shape_states :789 / set_shape_states :832: float[14S] = pos3, prevPos3, quat4, prevQuat4 */
int fs_add_sphere(fs_ctx *ctx, int env, float radius, const float *pos3, const float *quat4);
int fs_clear_shapes(fs_ctx *ctx, int env);
int fs_get_shape_states(fs_ctx *ctx, int env, float *out, int n_floats);
int fs_set_shape_states(fs_ctx *ctx, int env, const float *in, int n_floats);

/* camera.  get_camera_params :891 -> [w,h,px,py,pz,ax,ay,az]; set_camera_params :908 <- [px,py,pz,ax,ay,az,w,h] */
int fs_get_camera_params(fs_ctx *ctx, int env, float *out8);
int fs_set_camera_params(fs_ctx *ctx, int env, const float *in8);

/* pyflex.render (pyflex.cpp:924-1133): RGBA8 bottom-up [h*w*4] and linear depth [h*w] of env. */
int fs_render(fs_ctx *ctx, int env, unsigned char *rgba, int n_bytes, float *depth, int n_floats);

/* white-box access for tests: the triangle meshes fs_render rasterises for env's kinematic spheres = what the reference
   draws for them (main.cpp:1739-1751: CreateSphere(20, 20, r) core/mesh.cpp:858-902, transformed by the shape's PREVIOUS
   position and rotation).  verts / normals: float[4 * 441 * S], tris: int[3 * 800 * S]; any of them may be null. */
int fs_get_sphere_mesh(fs_ctx *ctx, int env, float *verts, float *normals, int n_floats, int *tris, int n_ints);

/* white-box access for tests: renders env exactly as fs_render does and copies out what the passes left behind instead of the
   picture.  zkeys[w * h] (rows bottom-up like the picture): the camera pass's z-buffer, depth24 << 32 | primitive id, where
   depth24 = floor(window depth * (2^24 - 1) + 1/2) and ids run in draw order (1 .. 800 S: sphere triangles, then the cloth
   triangles; the ground plane, id 0, is intersected per pixel in the shading pass and is NOT in this plane); all ones where
   no triangle landed.  shadow[2048 * 2048]: the light's depth24 map after polygon offset, all ones where cleared.
   Either pointer may be null; same argument checks as fs_render.  Never on a hot path. */
int fs_get_render_buffers(fs_ctx *ctx, int env, unsigned long long *zkeys, long long n_keys, unsigned int *shadow,
                          long long n_texels);

/* coverage reward of every env (flex_utils.py:358-395 get_current_covered_area with pos=None, particle radius
   0.00625), out[n_envs] in float64 like the reference's return value; envs without a scene report 0. */
int fs_coverage(fs_ctx *ctx, double *out, int n_doubles);

/* white-box access for tests: particle-contact candidate lists of the last substep, counts[N], lists[N*96] */
int fs_get_last_neighbors(fs_ctx *ctx, int env, int *counts, int *lists);
/* white-box access for tests: the collideShapes stage of the last substep (NvFlex.h:205; candidates within collisionDistance +
   shapeCollisionMargin of the predicted position, NvFlex.h:145-147, at most maxContactsPerParticle, NvFlex.h:361), masks[N]:
   bit q = plane q, bit 8 + q = kinematic sphere q */
int fs_get_last_shape_candidates(fs_ctx *ctx, int env, unsigned *masks);
/* white-box access for tests: which kernel form the most recent fs_step* launch of this context ran (0 = none yet).
   The launch size selects the form (fs_solver.hip), so a parity test asserts that it compared the form it meant to. */
#define FS_FORM_FUSED_12 1       /* fs_k_fused_step<12>: register-resident coded adjacency, <= 12 springs per particle */
#define FS_FORM_FUSED_16 2       /* fs_k_fused_step<16>: the same with <= 16 springs per particle */
#define FS_FORM_FUSED_GENERIC 3  /* fs_k_fused_step<0>: adjacency streamed from the ELL arrays */
#define FS_FORM_STREAM_EAGER 4   /* fs_k_iterate_eager<false>: latency form of small launches */
#define FS_FORM_STREAM_CODED 5   /* fs_k_iterate<true>: throughput form, one-byte spring codes */
#define FS_FORM_STREAM_ELL 6     /* fs_k_iterate<false>: throughput form, uncompressed adjacency */
#define FS_FORM_STREAM_GRID 7    /* fs_k_iterate_grid: neighbour ids from the grid coordinates (large launches) */
#define FS_FORM_STREAM_GRIDL 9   /* fs_k_iterate_gridl: canonical grid cloths, rest lengths from the per-particle table */
#define FS_FORM_FUSED_GRID64 8   /* fs_k_fused_grid64: 64-wide grid cloths, packed two-particle springs, no adjacency */
#define FS_FORM_STREAM_GRIDL_TP 10 /* fs_k_iterate_gridl_tp: the grid-L iteration's throughput form -- launches above 262 144 particles of
                                      tether-free cloths (the evaluation loop at its real sizes): springs in two halves of six,
                                      equal-mass fast path */
#define FS_FORM_STREAM_MESH 11   /* fs_k_iterate_mesh: throughput form of cloths without stream codes, packed mesh words (one
                                    8-byte load per spring slot instead of three 4-byte loads) */
#define FS_FORM_STREAM_MIXED 12  /* fs_k_iterate_mixed: every workgroup runs the body its slot's cloth allows (GRIDL_TP, CODED,
                                    MESH or ELL: fs_last_slot_forms) */
int fs_last_kernel_form(const fs_ctx *ctx);
/* white box: the FS_FORM_* of every list position of the most recent streaming launch -- FS_FORM_STREAM_GRIDL_TP, _CODED, _MESH
   or _ELL inside an FS_FORM_STREAM_MIXED launch, the launch's own form otherwise.  Computed on the host from the episodes'
   descriptors (also for a caller's device list, where retired positions keep the form of the episode they held).  Writes at
   most `cap` entries and returns the number of list positions. */
int fs_last_slot_forms(const fs_ctx *ctx, int *forms, int cap);
/* white box: how the most recent streaming launch did its substep boundaries (finalize + predict + bucket sort): 0 = four
   kernels (launches of fewer than 16 episodes, cloths above 16384 particles), 1 = fs_k_boundary (one launch per boundary) */
int fs_last_boundary_form(const fs_ctx *ctx);
/* Streaming back-end: a launch list that cannot fill the chip is split into `groups` slot ranges whose launch chains run
   concurrently on streams of their own (episodes are independent; results do not change).  0 = the library's measured
   default (1 below ~24 x 4096 particles, 2 from there), 1..4 = forced.  fs_last_stream_groups: the
   number of chains of the most recent streaming launch (white box for the tests). */
int fs_set_stream_groups(fs_ctx *ctx, int groups);
int fs_last_stream_groups(const fs_ctx *ctx);
/* white-box access for tests: y[i] = the reciprocal square root the constraint kernels use (csrc/fs_constraints.h fs_rsqrt),
   evaluated on the device for n host values -- what pins the checker's restatement of it to this chip */
int fs_eval_rsqrt(fs_ctx *ctx, const float *x, float *y, int n);
/* device pointer of env's position array (float4[N]) for zero-copy consumers (torch) */
void *fs_device_positions(fs_ctx *ctx, int env);

/* ---- episode fork (additive: the reference runs one cloth per process and cannot branch) ---------------------------------
   Copy the complete simulation state of episode src[k] into slot dst[k], k < n.  One src may feed several dst.  Afterwards
   dst[k] is indistinguishable from src[k] to every solver form, picker call, reduction and render: the same sequence of calls
   on both leaves identical bits, and stepping one never changes the other.
   Shared: the device topology.  Copied: the host scene; positions (with the inverse masses a grasp zeroed), velocities,
   phases; the parameter table (fs_set_params); the shapes with their previous poses and rotations; the picker state (held
   particles, saved inverse masses, thresholds, radius, whether fs_picker_reset ran); camera and the phase summary.
   NOT copied: per-substep scratch (every frame rewrites it before reading it -- so fs_get_last_neighbors /
   fs_get_last_shape_candidates of a forked slot are defined only after its first step); the snapshot of
   fs_snapshot_positions (the destination has none: take one before fs_max_displacement); capture (the destination starts
   with capture off, frames it had not handed over stay); the destination's wait / step loop state of fs_advance is reset.
   A scene dst[k] held before is released as fs_set_scene releases it; the slab comes from the context's buffer pool.
   The particle arrays of all pairs move in ONE launch on the context's current stream (pairs grouped by source: a source
   tile is read once and stored to each of its destinations, 16-byte accesses); the call does not wait for it -- every getter
   synchronises.  The host waits only for a PREVIOUS fs_fork's table upload and, when a destination held a scene, for the
   work that may still use its old slab.
   Refused before anything is launched: FS_ERR_ARG for n < 1, a null list, an index outside the context, src[k] == dst[k], a
   slot that is both a source and a destination, a destination listed twice; FS_ERR_STATE for a source without a scene and,
   on the service lane, for any listed slot that belongs to a chunk in flight (fs_service_lane's contract). */
int fs_fork(fs_ctx *ctx, int n, const int *src, const int *dst);

/* ---- on-device picker + movep executor (additive) -------------------------------------------
   Native counterpart of the host loop the reference runs around pyflex.step(): SimEnv.movep (simEnv.py:739-769) ->
   PickerPickPlace.step (flex_utils.py:223-252) -> Picker.step (flex_utils.py:121-205).  The pickers are the
   episode's kinematic spheres (fs_add_sphere); results are identical to driving fs_step through those Python classes. */
/* Picker.reset bookkeeping (flex_utils.py:85,99-101): nothing held; remember every particle's inverse mass. */
int fs_picker_reset(fs_ctx *ctx, int env, double picker_threshold, double particle_radius);
/* Picker.picker_radius (flex_utils.py:57) as the python float the reference adds into the grasp threshold
   (flex_utils.py:154-155); without this call the threshold uses the float32 radius pyflex.add_sphere stored for shape 0.
   fs_picker_reset clears it. */
int fs_picker_set_radius(fs_ctx *ctx, int env, double picker_radius);
/* simulation steps, summed over the episodes, that the most recent fs_movep / fs_movep_batch* call -- or the movep
   entries of the most recent fs_advance call -- executed (movep iterations that find the pickers on their targets do not
   step the simulation, flex_utils.py:231-233); 0 after a call that returned an error before launching anything */
long long fs_last_movep_steps(const fs_ctx *ctx);
/* One chunk (at most `cap` simulation steps) for episodes that are in different phases of their primitives, so that all of
   them share every launch sequence; the chunk ends with the first movep that completes, but takes at least cap_min steps
   (one host round trip per call) when somebody has that many left: kind[a] = 0: SimEnv.movep (simEnv.py:739-769) towards targets[a] ([S][3], float64; f32[a]
   != 0: the caller's targets were a float32 array, see fs_movep_batch_f32) with grasp[a][S], speed[a], iteration limit[a],
   min_steps[a] (< 0: None), resumed at loop iteration start[a]; kind[a] = 1: flex_utils.wait_until_stable
   (flex_utils.py:430-441) with max_steps = limit[a], of which start[a] steps are already taken, tolerance tolerance[a];
   kind[a] = 2: limit[a] plain pyflex.step() calls, start[a] of them taken (status 1 when done).
   Out: progress[a] = loop iteration / step count reached (pass it back as start[a]), status[a] = 0 continue with another
   call, 1 finished (targets reached / stable), 2 finished at the limit (movep: MoveJointsException; wait: not stable),
   steps[a] = simulation steps this call took for the episode.  Results are identical to the uninterrupted loops. */
int fs_advance(fs_ctx *ctx, int n, const int *envs, const int *kind, const double *targets, const int *grasp,
               const double *speed, const int *limit, const int *min_steps, const int *f32, const int *start, double eps,
               const double *tolerance, int cap_min, int cap, int *progress_out, int *status_out, int *steps_out);
/* fs_advance in two halves, so that the host can work while a chunk runs (flingbot_amd/schedule.py pipelines them: the
   next chunk is queued, and the requests of the episodes that just finished something are served, while the device is
   still busy with the previous one).
   fs_advance_begin: same arguments; queues the chunk's launches on the context's main stream and returns a ticket (>= 0; at
   most 4 may be open) or an error code (< 0).  The movep entries' outputs are final when it returns -- their trajectories
   are planned on the host -- and so are those of a wait / step loop whose steps were already used up; every other wait /
   step entry has status -1 until fs_advance_end.  start[a] = -1 for a wait / step entry CONTINUES the loop from the state
   the device keeps per episode: the host may queue the next chunk of a wait before it knows whether the previous chunk
   ended it (if it did, the episode's entries retire at once and nothing is stepped).
   fs_advance_end: waits for the ticket's launches and fills in the wait / step entries (same index a as in the begin
   call; progress = steps of the loop taken so far, steps = progress - start, or -1 for start = -1).
   fs_advance_in_flight: open tickets. */
int fs_advance_begin(fs_ctx *ctx, int n, const int *envs, const int *kind, const double *targets, const int *grasp,
                     const double *speed, const int *limit, const int *min_steps, const int *f32, const int *start, double eps,
                     const double *tolerance, int cap_min, int cap, int *progress_out, int *status_out, int *steps_out);
int fs_advance_end(fs_ctx *ctx, int ticket, int *progress_out, int *status_out, int *steps_out);
int fs_advance_in_flight(const fs_ctx *ctx);
/* The service lane: between fs_service_lane(ctx, 1) and fs_service_lane(ctx, 0) every entry point of the library works on
   a second, high-priority stream, so that reductions, observations and resets for episodes that are NOT part of a chunk
   in flight neither queue up behind the chunk nor wait for it.  Contract: on the lane the caller touches only such
   episodes (or ones whose wait loop in the chunk has already ended).  Leaving the lane orders the main stream behind it.
   The calls that REWRITE an episode (fs_set_scene*, fs_set_positions / velocities / phases / params / shape_states /
   particles, fs_add_sphere, fs_clear_shapes, fs_picker_reset) check the contract: FS_ERR_STATE for an episode that an open
   ticket still steps or moves (an entry that continues a wait loop fs_advance_end has already reported over does not count).
   The calls that STEP the simulation (fs_step, fs_step_list, fs_step_timed, fs_wait_until_stable, fs_movep*, fs_advance*)
   return FS_ERR_STATE on the lane while any ticket is open, whichever episodes they list: a launch sequence uses per-context
   tables and streams the chunk in flight is still reading. */
int fs_service_lane(fs_ctx *ctx, int on);
/* fs_advance's stopwatch since fs_create: out5 = calls, launch sequences, wall ms inside the calls, device ms between a
   call's first and last launch, wall ms the calls spent before their first launch (planning, tables, upload) */
int fs_advance_timing(const fs_ctx *ctx, double *out5);
/* The context's buffer pool (episode slabs, topology images, ticket tables: recycled by size instead of hipFree / hipMalloc,
   which synchronise the device).  out[0] = idle bytes held, out[1] = idle buffers, out[2] = the idle limit in bytes: what
   lies beyond it goes back to the driver, oldest first (4 GiB; FLINGSIM_POOL_IDLE_MB overrides it when the library loads). */
int fs_pool_stats(const fs_ctx *ctx, long long *out3);
/* picked particle index per picker (-1 = none) */
int fs_picker_get_picked(fs_ctx *ctx, int env, int *out, int n_ints);
/* SimEnv.movep: move picker k toward targets[3k..3k+2] by `speed` per simulation step with grasp flag grasp[k], until all
   are within eps (and more than min_steps iterations ran; min_steps < 0 = None).  Runs every simulation step on the
   device without host round trips.  iterations_out = loop iterations (what movep's `step` counts).
   Returns FS_ERR_LIMIT when `limit` iterations were not enough. */
int fs_movep(fs_ctx *ctx, int env, const double *targets, const int *grasp, double speed, int limit, int min_steps,
             double eps, int *iterations_out);
/* the same for n episodes at once: targets double[n][S][3], grasp int[n][S], iterations_out int[n] */
int fs_movep_batch(fs_ctx *ctx, int n, const int *envs, const double *targets, const int *grasp, double speed, int limit,
                   int min_steps, double eps, int *iterations_out);
/* the same when the reference's `pos` argument is a float32 numpy array (stretch_cloth builds its targets from the
   float32 picker positions, simEnv.py:146-156,180-182): movep's own arithmetic then runs in float32 */
int fs_movep_batch_f32(fs_ctx *ctx, int n, const int *envs, const float *targets, const int *grasp, double speed,
                       int limit, int min_steps, double eps, int *iterations_out);

/* ---- frame capture during movep (additive) --------------------------------------------------------------------------
   The reference's `--dump_visualizations`: while a picker moves, SimEnv.movep appends get_image()[0] -- the colour part of
   pyflex.render(), rows flipped to top-down, alpha dropped (flex_utils.py:418-427) -- to env_video_frames['top'] after every
   loop iteration `step` with step % 4 == 0 (simEnv.py:764-768), also when PickerPickPlace.step returned without stepping the
   simulation (flex_utils.py:231-233), never in the iteration that finds the pickers on target and returns.  fs_movep* and
   fs_advance* run all steps of a trajectory on the device, so the frames are taken there: for an episode with capture on,
   the capture form of the renderer is queued right behind the launch sequence of the step a frame follows (same stream, no
   host synchronise), into a frame store that belongs to the call (to the ticket, for fs_advance_begin); one asynchronous
   copy to pinned memory follows the call's last launch.  After fs_movep* returns / after fs_advance_end the frames are on the
   host, in order (close tickets in the order they were opened).  wait_until_stable and plain steps are never filmed
   (the reference films in movep only).  Episodes without capture cost nothing: no launch, copy or allocation.
   fs_capture_enable: frames of `width` x `height` (a render at that size with the episode's camera pose, not a resampled
     one) from now on; allocates the episode's private render scratch (z-buffer, 2048^2 shadow map, normals, sphere meshes),
     sized for its current scene.  fs_set_scene switches capture OFF again (a new scene ends the old film; frames not yet
     taken stay), and enabling at another frame size drops whatever frames are still waiting.  What SimEnv.reset does by
     emptying env_video_frames after its own reset_end_effectors (simEnv.py:677-681) is: enable after those.
   fs_capture_disable: stop; frames not yet taken stay.  Both are refused (FS_ERR_STATE, before any HIP call) for an episode
     that a chunk in flight films, and on the service lane for one that a chunk in flight moves (fs_service_lane's contract).
   fs_capture_count: frames waiting.  fs_capture_size: returns 1 / 0 = capture on / off, and the frame size.
   fs_capture_take: copies the waiting frames (uint8 [count][height][width][3]) into out[n_bytes], forgets them and returns
     their number (what SimEnv.on_episode_end does with the list, simEnv.py:791-803). */
int fs_capture_enable(fs_ctx *ctx, int env, int width, int height);
int fs_capture_disable(fs_ctx *ctx, int env);
int fs_capture_count(const fs_ctx *ctx, int env);
int fs_capture_size(const fs_ctx *ctx, int env, int *width, int *height);
int fs_capture_take(fs_ctx *ctx, int env, unsigned char *out, long long n_bytes);

/* ---- per-episode appearance (additive) ----------------------------------------------------------------------------------
   The reference's paper configuration renders through Blender with domain randomisation (README.md:178-184): every render
   call draws a fresh cloth colour and a fresh slice of a noise texture on the ground (render_rgbd.py:26-37).  The renderer
   here takes both from the episode's fs_appearance; the default is what the OpenGL path draws (one pink cloth, a black
   ground).  The cloth colour is the reference's notion; the ground texture is this project's own rule, stated below and in
   csrc/fs_raster_kernels.h.  Host-side state: neither call allocates, launches or synchronises anything; every render of
   the episode that is QUEUED afterwards (fs_render, fs_observe*, capture frames) uses the new value.
   Ground texture (ground_octaves = O > 0), at the point (hx, hz) where the pixel's ray meets the ground, fp32 throughout:
     for o = 0 .. O-1:  f = ground_cells_per_m * 2^o;  u = clamp(hx f, -2^30, 2^30), v = clamp(hz f, -2^30, 2^30);
                        i = floor(u), j = floor(v) (as 32-bit integers);  a = u - i, b = v - j;  s(x) = x^2 (3 - 2 x);
                        L(i, j) = (hash(i, j, o, seed) >> 8) * 2^-24;
                        n_o = (L(i,j) (1 - s(a)) + L(i+1,j) s(a)) (1 - s(b)) + (L(i,j+1) (1 - s(a)) + L(i+1,j+1) s(a)) s(b)
     t = (sum_o n_o 2^-(o+1)) / (1 - 2^-O);   albedo = ground_rgb[0] + (ground_rgb[1] - ground_rgb[0]) t
     hash(i, j, o, seed), all in wrapping 32-bit unsigned arithmetic (i, j reinterpreted from two's complement):
       h = i * 0x9E3779B1 + j * 0x85EBCA77 + o * 0xC2B2AE3D + seed
       h ^= h >> 16;  h *= 0x7FEB352D;  h ^= h >> 15;  h *= 0x846CA68B;  h ^= h >> 16
   The albedo goes through the unchanged shader (shadow, spot, ambient, fog, gamma).  One point sample at the pixel centre,
   no filtering: the setter caps the finest octave at 256 cells per metre, about two pixels per cell at 720^2 under the
   default camera.  ground_octaves = 0: the flat ground_rgb[0], shaded by the kernels every render ran before.
   fs_set_appearance: table[k] becomes the appearance of episode envs[k].  Refused with FS_ERR_ARG, before ANY episode is
     changed: a null argument, n < 1, an index outside the context, an episode without a scene, a non-finite or negative
     albedo, ground_octaves outside 0 .. 6, and with ground_octaves > 0 a ground_cells_per_m that is not finite, <= 0 or
     whose finest octave ground_cells_per_m * 2^(ground_octaves - 1) exceeds 256.  Refused with FS_ERR_STATE (as
     fs_capture_enable is): an episode that a chunk in flight films -- its frames are being shaded.
   fs_set_scene / fs_set_scene_prebuilt put the default back (a new scene is a new episode); fs_fork copies the source's
   appearance to every destination.
   fs_get_appearance: the episode's current value (the default for an episode without a scene).
   fs_appearance_default: the default into *out (may be null); returns sizeof(fs_appearance).
   fs_appearance_check: the setter's checks of ONE value without a context: FS_OK, or FS_ERR_ARG with a message. */
typedef struct fs_appearance {
    float cloth_rgb[3];        /* linear albedo; default 0.612f*1.5f, 0.194f*1.5f, 0.394f*1.5f */
    float ground_rgb[2][3];    /* linear albedo where the noise is 0 / 1; default 0.001f everywhere */
    unsigned ground_seed;
    float ground_cells_per_m;  /* lattice cells per metre of octave 0 */
    int ground_octaves;        /* 0: flat ground_rgb[0] (default); 1..6: fractal value noise */
} fs_appearance;
int fs_set_appearance(fs_ctx *ctx, int n, const int *envs, const fs_appearance *table);
int fs_get_appearance(fs_ctx *ctx, int env, fs_appearance *out);
int fs_appearance_default(fs_appearance *out);
int fs_appearance_check(const fs_appearance *a);
/* The texture rule on the host, without a context or a GPU (the function the shading kernels inline, compiled for the
   CPU): t[k] of the rule at the ground point (hx[k], hz[k]); 0 everywhere for ground_octaves = 0. */
int fs_host_ground_texture(const fs_appearance *a, int n, const float *hx, const float *hz, float *t);
/* The half-stencil neighbour search of the grid-64 kernel on the host, without a context or a GPU (the enumeration rule
   the kernel includes, compiled for the CPU).  pos4: float[4 * n]; bucket_bits: log2 of the hash size (the kernel ships
   13); dimx > 0: stencil filter of a canonical grid cloth of that width, 0: every pair.  counts[n], lists[n * ncap]
   (ascending, the ncap smallest, -1 padded), facts[4] = {alias hits rejected, wrapped runs, particles over the cap,
   longest list before truncation} (may be NULL). */
int fs_host_pair_search(int n, const float *pos4, float radius, int bucket_bits, int ncap, int dimx, int *counts,
                        int *lists, int *facts);

/* ---- device-side feedback loops and reductions -------------------------------------------------
   The reference's primitives download whole particle arrays to take one number from them, every simulation step or
   every loop trip; these entry points compute the same numbers on the device.                                        */
/* flex_utils.py:430-441 wait_until_stable for n episodes at once: before EVERY step the episode's max |velocity
   component| (float32, compared in double like `np.abs(v).max() < tolerance`) is tested; an episode that passes stops
   stepping.  At most max_steps steps.  steps_out[k] = simulation steps taken, stable_out[k] = 1 when the test passed
   (the function's return value), 0 when max_steps ran out.  No host round trip per step. */
int fs_wait_until_stable(fs_ctx *ctx, int n, const int *envs, int max_steps, double tolerance, int *steps_out,
                         int *stable_out);
/* out[3k..3k+2] = { min height y, max height y, max |velocity component| } of episode envs[k]
   (simEnv.py:186-200 lift_cloth `heights.min()`, :809-813 is_cloth_grasped `heights.max()`, flex_utils.py:435) */
int fs_cloth_stats(fs_ctx *ctx, int n, const int *envs, float *out, int n_floats);
/* stretch_cloth's probe (simEnv.py:155-168) for episode envs[k]:
     single_grasp_out[k] = 1 when every particle with y > height_thr[k] has x < 0, or every one has x > 0 (also when there
                           is none), evaluated in float32 like the numpy expression;
     nearest_out[3k..]   = position of the particle whose float32 distance to midpoint_xz[2k..2k+1] in the x-z plane,
                           sqrt(dx*dx + dz*dz), is smallest (lowest index on ties = Python's stable sort). */
int fs_stretch_probe(fs_ctx *ctx, int n, const int *envs, const float *midpoint_xz, const float *height_thr,
                     int *single_grasp_out, float *nearest_out);
/* SimEnv.preaction / postaction (simEnv.py:464-475): keep the current positions of the listed episodes on the device,
   and later report out[k] = max_i || |pos_i - kept_i| ||_2 in float32 -- np.linalg.norm(np.abs(post - pre), axis=1).max() --
   which the reference compares with 5e-2 to end an episode whose action did not move the cloth.  A list with a bad id or
   a scene-less episode is refused as a whole: no listed episode's snapshot is replaced. */
int fs_snapshot_positions(fs_ctx *ctx, int n, const int *envs);
int fs_max_displacement(fs_ctx *ctx, int n, const int *envs, float *out, int n_floats);
/* Write ONE particle per listed episode: position + inverse mass from pos4[4k..4k+3], velocity zeroed when zero_velocity != 0.
   The reference's task generator (environment/tasks.py:177-224) moves a pinned pick point by reading and rewriting the
   whole position and velocity arrays through pyflex every simulation step. */
int fs_set_particles(fs_ctx *ctx, int n, const int *envs, const int *particle_ids, const float *pos4, int zero_velocity);

/* ---- particle state as batched device tensors (additive: the reference moves particle arrays one episode at a time through
   host memory) -------------------------------------------------------------------------------------------------------------
   fs_state_gather packs the state of episodes envs[0 .. n-1] into padded device arrays, ONE launch for all listed episodes
   and all requested fields:
     d_pos4  float32 [n][n_max][4]   x, y, z, inverse mass exactly as stored (with the zeros a grasp wrote)
     d_vel4  float32 [n][n_max][4]   x, y, z and the fourth lane as stored
     d_phase int32   [n][n_max]
   all contiguous and on the context's device, d_pos4 / d_vel4 on 16-byte boundaries; any of the three may be null, not all.
   Row k holds episode envs[k]: particles 0 .. N_k-1 in the episode's own order, rows N_k .. n_max-1 written as ZEROS -- every
   byte of an output is written, none depends on what the array held before.  counts[k] = N_k (host output, may be null).
   Episodes may repeat and come in any order.
   Ordering: the launch runs on the context's current stream behind everything queued there (a gather right after fs_step_list
   sees the stepped state); the call RETURNS WHEN ITS LAUNCH HAS FINISHED, so the arrays may be used on any stream at once.
   (Handing over an event instead of waiting is a later change.)  The caller makes sure nothing on another stream still uses
   the arrays when the call is made.
   Refused as a whole with FS_ERR_ARG, the reason in fs_last_error, nothing launched: a null context / list, n < 1, all three
   arrays null, a misaligned array, an id outside the context, a slot without a scene, n_max below the largest N_k. */
int fs_state_gather(fs_ctx *ctx, int n, const int *envs, int n_max, float *d_pos4, float *d_vel4, int *d_phase, int *counts);
/* The way back: rows 0 .. N_k-1 of d_pos4 and / or d_vel4 (layout as above, either may be null, not both) become the
   positions with inverse masses / the velocities of episode envs[k], one launch for all of them.  Per episode this is
   fs_set_positions / fs_set_velocities: the fourth velocity lane is stored as 0 whatever the array holds, nothing else of the
   episode changes, and on the service lane a listed episode that belongs to a chunk in flight is refused with FS_ERR_STATE
   (fs_service_lane's contract).  Rows at or beyond N_k are not read.  Same ordering and completion rule as fs_state_gather:
   behind everything queued on the context's current stream, returns when the launch has finished.
   Refused with FS_ERR_ARG besides fs_state_gather's reasons: a destination listed twice.  A refusal of either kind leaves
   every listed episode untouched. */
int fs_state_scatter(fs_ctx *ctx, int n, const int *envs, int n_max, const float *d_pos4, const float *d_vel4);

/* ---- observation transforms on the device ---------------------------------------------------
   learning/nets.py:155-193 prepare_image: n_transforms rotated / scaled / resized copies of one observation.
     d_img   device float32 [channels][size][size]                  (the tensor preprocess_obs returns)
     matrix  host double [n][4], offset host double [n][2]          rotation matrix rows and offset exactly as
             scipy.ndimage.rotate(reshape=False) derives them from the angle (c, s = cosdg, sindg; [[c, s], [-s, c]];
             offset = centre - matrix @ centre) -- computed by the caller so special angles stay exact
     scale   host double [n]                                        <1 centre crop, >1 replicate pad to int(scale*size)
     d_out   device float32 [n][channels][dim][dim]
     d_work  device scratch of fs_prepare_image_work_bytes() bytes; stream: hipStream_t the work is enqueued on
   Cubic-spline rotation (mode='nearest', float64 like scipy) evaluated only at the pixels the nearest-neighbour resize
   keeps. */
size_t fs_prepare_image_work_bytes(int channels, int size, int n_transforms);
int fs_prepare_image(const float *d_img, int channels, int size, int n_transforms, const double *matrix,
                     const double *offset, const double *scale, int dim, float *d_out, void *d_work, void *stream);

/* ---- action selection on the device ----------------------------------------------------------
   SimEnv.get_max_value_valid_action (environment/simEnv.py:560-661): the best-valued VALID action over all primitives,
   transforms and pixels.  A candidate (primitive p, transform t, pixel (y, z)) is valid when its two reach points lie
   in the obs_dim image (get_action_params :517-537), map into the pretransform image (pixels_to_3d_positions,
   environment/utils.py:237-276, with `transform_mats[t]` = get_transform_matrix(depth_dim, obs_dim, -rotation, scale)
   row-major), unproject through `d_depth` (pixel_to_3d :214-234) and satisfy check_action_reachability (:539-558;
   stretchdrag also at the end of its drag :624-642).
     d_values  device float32 [n_primitives][n_transforms][obs_dim][obs_dim] (stacked value maps)
     best_index_out  flattened index into values[:, :, g:-g, g:-g] (g = pix_grasp_dist) of the winner -- the entry the
                     reference's descending walk stops at (ties: lowest flattened index) -- or -1 when nothing is valid
     d_work    device scratch of fs_select_action_work_bytes(n_transforms) bytes; stream: hipStream_t */
#define FS_ACTION_FLING 0
#define FS_ACTION_STRETCHDRAG 1
#define FS_ACTION_DRAG 2
#define FS_ACTION_PLACE 3
#define FS_ACTION_MAX_PRIMITIVES 8
size_t fs_select_action_work_bytes(int n_transforms);
int fs_select_action(const float *d_values, int n_primitives, const int *primitive_kinds, int n_transforms, int obs_dim,
                     int pix_grasp_dist, int pix_drag_dist, int pix_place_dist, const double *transform_mats,
                     const float *d_depth, int depth_dim, double focal_length, const double *pose_matrix,
                     const double *left_arm_base, const double *right_arm_base, double reach_distance_limit,
                     double stretchdrag_dist, double grasp_height, long long *best_index_out, float *best_value_out,
                     void *d_work, void *stream);

/* The same validity (fs_act_valid, the same float64 expressions), reduced per (episode, primitive, transform) MAP instead of
   over everything, for n episodes in one call: the best valid candidate of every map.  Neighbouring pixels of one map have
   near-equal values, so an observation's K best pixels are K copies of one action; the winners of distinct rotation x scale
   maps are different actions (flingbot_amd/lookahead.py executes the K best of them side by side).
     d_values        device float32 [n][n_primitives][n_transforms][obs_dim][obs_dim], contiguous
     d_depth         device float32 [n][depth_dim][depth_dim], contiguous
     transform_mats  host double [n][n_transforms][9]: adaptive scales differ per episode
     index_out       host [n][n_primitives][n_transforms]: the winner's flattened index into values[:, :, g:-g, g:-g] OF ITS
                     EPISODE (fs_select_action's convention), -1 where no candidate of the map is valid; NaN values are skipped,
                     ties go to the lowest flattened index
     value_out       host [n][n_primitives][n_transforms]: the winner's value (0 where index_out is -1)
     d_work          fs_transform_winners_work_bytes(n, n_primitives, n_transforms) bytes of device scratch, 16-byte aligned
   The remaining arguments are fs_select_action's.  One table upload, one launch (one workgroup per map, reduced in LDS), one
   download; returns when the results are on the host.  For every episode the best entry of its row (value descending, index
   ascending) is what fs_select_action returns for that episode. */
size_t fs_transform_winners_work_bytes(int n, int n_primitives, int n_transforms);
int fs_transform_winners(const float *d_values, int n, int n_primitives, const int *primitive_kinds, int n_transforms,
                         int obs_dim, int pix_grasp_dist, int pix_drag_dist, int pix_place_dist, const double *transform_mats,
                         const float *d_depth, int depth_dim, double focal_length, const double *pose_matrix,
                         const double *left_arm_base, const double *right_arm_base, double reach_distance_limit,
                         double stretchdrag_dist, double grasp_height, long long *index_out, float *value_out, void *d_work,
                         void *stream);

/* The same validity once more, per CELL instead of behind a reduction: a lattice of pixels of chosen maps, every cell with
   its own answer (flingbot_amd/probe.py executes the valid cells of one map side by side, each on a fork of the episode).
   The cells of request k are the pixels (y0 + i stride, z0 + j stride), 0 <= i < gy, 0 <= j < gz, of the map (episode,
   primitive, transform); cell (i, j) is entry i gz + j of row k of the outputs.
     requests   host [m], m in 1 .. 65535; stride >= 1, gy gz in 1 .. 4096, every cell inside [0, obs_dim)
     conservative_grasp_radius   r of BatchedFlingEnv._on_cloth, in pixels of the depth plane
     code_out   host uint8 [m][pitch], pitch = the largest gy gz of the table (every row as long as the longest lattice;
                entries past a shorter one are 0):
                bit 0   fs_act_valid, as fs_select_action and fs_transform_winners evaluate it (the same float64 expressions)
                bit 1   grasp point 1 is on cloth: every pixel (row, column) of the episode's depth plane with
                        (row - b)^2 + (column - a)^2 <= r^2 (integers) inside the image has depth != 2.0f, where (a, b) is the
                        point's pretransform pixel -- read, as everywhere, as column a, row b; r <= 0: on cloth
                bit 2   the same for grasp point 2
                bits 1 and 2 are 0 where bit 0 is 0
     value_out  host float32 [m][pitch]: the map's value at the cell, NaN included, whatever the code says (0 past a shorter
                lattice)
     d_work     fs_lattice_actions_work_bytes(n, n_transforms, m, pitch) bytes of device scratch, 16-byte aligned
   The remaining arguments are fs_transform_winners'.  One table upload (matrices and requests), one launch (one workgroup
   per request, cells strided over its threads), one download; returns when the results are on the host.  Refused with
   fs_last_error before anything is enqueued: null pointers, m, stride, gy gz or a cell out of range, an episode, primitive or
   transform that does not exist, a misaligned d_work. */
typedef struct fs_lattice_request {
    int episode, primitive, transform, y0, z0, stride, gy, gz;
} fs_lattice_request;
size_t fs_lattice_actions_work_bytes(int n, int n_transforms, int m, int max_cells);
int fs_lattice_actions(const float *d_values, int n, int n_primitives, const int *primitive_kinds, int n_transforms,
                       int obs_dim, int pix_grasp_dist, int pix_drag_dist, int pix_place_dist, const double *transform_mats,
                       const float *d_depth, int depth_dim, double focal_length, const double *pose_matrix,
                       const double *left_arm_base, const double *right_arm_base, double reach_distance_limit,
                       double stretchdrag_dist, double grasp_height, const fs_lattice_request *requests, int m,
                       int conservative_grasp_radius, unsigned char *code_out, float *value_out, void *d_work, void *stream);

/* K DISTINCT valid actions per observation, drawn without replacement with probability proportional to exp(value / tau) over
   all primitives x transforms x pixels (Gumbel-top-K: one perturbation per candidate, the K largest perturbed keys are a
   Plackett-Luce draw).  Stateless and batched over n observations like fs_transform_winners, whose arguments it takes;
   fs_act_valid and the on-cloth rule of fs_lattice_actions are used as they are.  Nothing of this is in the reference.
     candidates      flat index c in [0, P T W W), W = obs_dim - 2 g, decoded as fs_select_action decodes it; refused when the
                     total reaches 2^31
     k               picks per observation, 1 .. 16
     d_noise         device float32 [1 << noise_bits], noise_bits must be 16: the perturbation table (for a Gumbel draw
                     -log(-log((i + 0.5) / 65536))).  An input, so that the device's arithmetic is IEEE add and multiply only
     inv_tau         float32 1 / tau, finite and >= 0 (0: a uniform draw over the eligible candidates)
     sample_keys     host uint32 [n][2]: (key_lo, key_hi) of every observation
     eligible        the value is not NaN and fs_act_valid holds; for SAMPLED picks with on_cloth = 1 also: the primitive's
                     grasp points are on cloth -- bit 1 / bit 2 of fs_lattice_actions with radius conservative_grasp_radius
                     (r <= 0: on cloth), both points for fling and stretchdrag, the first point only for drag and place
     key(c)          fadd(fmul(value, inv_tau), d_noise[h(c) >> 16]), two float32 roundings, never one fused multiply-add; a
                     candidate whose key is NaN (an infinite value with inv_tau = 0) is skipped
     h(c)            uint32, wrapping: h = c 0x9E3779B1 + key_lo 0x85EBCA77 + key_hi 0xC2B2AE3D; h ^= h >> 16; h *= 0x7FEB352D;
                     h ^= h >> 15; h *= 0x846CA68B; h ^= h >> 16 (the ground texture's finaliser).  It does not depend on the
                     pick number
     pick 0 with first_greedy = 1   the eligible candidate (no on-cloth filter) with the largest raw VALUE, ties to the lowest
                     index: fs_select_action's winner for that observation
     every other pick   the eligible candidate with the largest key, ties to the lowest flat index, that is not SUPPRESSED: a
                     candidate is suppressed when an earlier pick (the greedy one included) has its primitive and both of its
                     pretransform pixels lie within Chebyshev distance `separation` (>= 0) of that pick's corresponding pixels
                     (separation = 0: no two picks with one primitive and pixel pair)
     index_out       host int64 [n][k]: flat indices, -1 from the first pick that found nothing
     value_out       host float32 [n][k]: the map's value at the pick, 0 where the index is -1
     key_out         host float32 [n][k]: the pick's key (a greedy pick: its value), 0 where the index is -1
     pix_out         host int32 [n][k][4]: the pretransform pixel pair (a0, a1, b0, b1), 0 where the index is -1
     d_work          fs_sample_actions_work_bytes(n, n_primitives, n_transforms, obs_dim, pix_grasp_dist, k) bytes of device
                     scratch, 16-byte aligned (the size call returns 0 for shapes the call refuses)
   One table upload (matrices and keys), two launches whatever n is (validity, on-cloth bit and key of every candidate once;
   then one workgroup per observation runs the k rounds, each a scan and an LDS arg-max), one download; returns when the
   results are on the host.  Refused with fs_last_error before anything is enqueued: null pointers, k outside 1 .. 16,
   noise_bits != 16, inv_tau negative or not finite, separation < 0, first_greedy or on_cloth other than 0 / 1, a misaligned
   d_work, 2^31 candidates or more. */
size_t fs_sample_actions_work_bytes(int n, int n_primitives, int n_transforms, int obs_dim, int pix_grasp_dist, int k);
int fs_sample_actions(const float *d_values, int n, int n_primitives, const int *primitive_kinds, int n_transforms,
                      int obs_dim, int pix_grasp_dist, int pix_drag_dist, int pix_place_dist, const double *transform_mats,
                      const float *d_depth, int depth_dim, double focal_length, const double *pose_matrix,
                      const double *left_arm_base, const double *right_arm_base, double reach_distance_limit,
                      double stretchdrag_dist, double grasp_height, int k, const float *d_noise, int noise_bits, float inv_tau,
                      const unsigned int *sample_keys, int first_greedy, int on_cloth, int conservative_grasp_radius,
                      int separation, long long *index_out, float *value_out, float *key_out, int *pix_out, void *d_work,
                      void *stream);

/* ---- observation stage on the device ---------------------------------------------------------
   Everything the reference does on the host between pyflex.render() and prepare_image, without downloading the frame:
   get_image (environment/flex_utils.py:418-427: flip rows, drop alpha, cv2.resize INTER_LINEAR to image_dim),
   SimEnv.get_cloth_mask (environment/simEnv.py:699-708: RGB2HSV, inRange((0,0,0),(100,100,100)) == 0, largest connected
   component, environment/utils.py:585-601), the bounding box SimEnv.get_obs derives its adaptive scale from
   (simEnv.py:717-731) and preprocess_obs (environment/utils.py:579-582).
     d_obs   device float32 [4][image_dim][image_dim]: rgb / 255 and depth, rows top-down
     d_mask  device uint8 [image_dim][image_dim] (1 = pixel of the largest cloth component) or NULL
     bbox    host int[5]: x.min, x.max, y.min, y.max of np.where(mask) (x = row) and the component's pixel count; -1 / 0
             when no pixel passes the colour test (the reference's get_obs then leaves the scale factors alone)
     d_work  device scratch of fs_observe_work_bytes(image_dim) bytes
   Renders with the episode's camera (fs_set_camera_params), runs on the context's stream and returns when the results are
   complete.  cv2 / skimage conventions are restated in oracle/observe.py (parity with the reference's own cv2 build is
   unpinned: cv2 is absent from the build image). */
size_t fs_observe_work_bytes(int image_dim);
int fs_observe(fs_ctx *ctx, int env, int image_dim, float *d_obs, unsigned char *d_mask, int *bbox, void *d_work);
/* fs_observe for n episodes with the host round trips of one call (the labelling rounds and the results of all
   episodes come back together).  d_obs [n][4][S][S], d_mask [n][S][S] or NULL, bbox [n][5],
   d_work: n * fs_observe_work_bytes(image_dim) bytes.  Every result equals the single call's. */
int fs_observe_batch(fs_ctx *ctx, int n, const int *envs, int image_dim, float *d_obs, unsigned char *d_mask, int *bbox,
                     void *d_work);
/* The same stage on n frames the caller supplies instead of rendering them: d_rgba[k] / d_depth[k] are device pointers in
   the renderer's layout (bottom-up RGBA bytes, widths[k] * heights[k] * 4, and float depth, widths[k] * heights[k]); the
   pointer and size arrays themselves live on the host.  Sizes may differ from frame to frame (each side 1..4096) and need not
   be square; a frame of exactly image_dim x image_dim is copied, every other one goes through the bilinear resize.
   d_obs, d_mask, bbox and d_work as for fs_observe_batch; runs on the context's stream, which must not race the
   producer of the frames.  fs_observe and fs_observe_batch are this call on the rasteriser's frames.
   On return of any of the three, the first n * image_dim * image_dim ints of d_work are the final labels of the n
   observations: -1 = the pixel fails the colour test, otherwise the raster index (row * image_dim + column) of the first
   pixel, in raster order, of the pixel's 8-connected component.  (The ints after them are scratch.) */
int fs_observe_frames(fs_ctx *ctx, int n, const unsigned char *const *d_rgba, const float *const *d_depth,
                      const int *widths, const int *heights, int image_dim, float *d_obs, unsigned char *d_mask, int *bbox,
                      void *d_work);

/* ---- value network forward ------------------------------------------------------------------
   SpatialValueNet.forward (learning/nets.py:81-141) in eval mode for size x size = 64 x 64 observations (the
   reference's obs_dim): normalise, Conv3x3(C->16)+BN+LeakyReLU, 8 residual blocks of two Conv3x3(16->16)+BN, Conv3x3(16->1).
   The caller folds each BatchNorm into the preceding convolution (w' = w g / sqrt(var + eps),
   b' = beta - running_mean g / sqrt(var + eps)) and packs the result once:
     fs_value_net_pack   host -> host.  in_channels 1 / 3 / 4; mean, std float32[in_channels] (preprocess_obs :131-137);
                         w_first [16][in_channels][3][3], b_first [16]; w_blocks [16 convs][16][16][3][3] in network order
                         (block 0 conv1, block 0 conv2, block 1 conv1, ...), b_blocks [16][16]; w_last [1][16][3][3];
                         packed float32[fs_value_net_param_floats()]
     fs_value_net_forward  d_params: the packed block copied to the device; d_obs device float32
                         [batch][obs_channels][64][64], of which channels channel_offset .. channel_offset+in_channels-1
                         feed the network (rgb_only: 0..2, depth_only: 3); d_out device float32 [batch][64][64];
                         d_work device scratch of fs_value_net_work_bytes(batch, 64) bytes; stream: hipStream_t.
                         d_params, d_obs, d_out and d_work must be 16-byte aligned (FS_ERR_ARG otherwise, before any
                         HIP call); d_work must not be in use by work queued on another stream.
   fp32 throughout (the 16->16 convolutions on v_mfma_f32_16x16x4_f32); any other size returns FS_ERR_ARG. */
size_t fs_value_net_param_floats(void);
size_t fs_value_net_work_bytes(int batch, int size);
int fs_value_net_pack(int in_channels, const float *mean, const float *std, const float *w_first, const float *b_first,
                      const float *w_blocks, const float *b_blocks, const float *w_last, float *packed);
int fs_value_net_forward(const float *d_params, const float *d_obs, int obs_channels, int channel_offset,
                         int in_channels, int batch, int size, float *d_out, void *d_work, void *stream);

/* ---- value network training: the three passes of a 16 -> 16 Conv3x3 (csrc/fs_vntrain.hip, nets.Conv16Function) ------
   fp32, NCHW-contiguous device tensors [batch][16][64][64], stride 1, zero padding 1, no bias; d_w is the layer's weight
   on the device in PyTorch's layout [16 oc][16 ic][3][3].
     fs_conv16_forward   transposed 0: d_y = conv3x3(d_x, W).  transposed 1: d_y = conv3x3(d_x, W') with
                         W'[ic][oc][tap] = W[oc][ic][8 - tap] -- the data gradient when d_x is the output gradient.
                         Not in place.  An image's result does not depend on the batch it is in (bit for bit).
     fs_conv16_wgrad     d_dw[oc][ic][ky][kx] = sum over b, y, x of d_g[b][oc][y][x] * d_x[b][ic][y+ky-1][x+kx-1], terms outside
                         the image zero.  d_work: fs_conv16_work_bytes(batch, 64) bytes of device scratch (per-strip partial
                         tiles, added by a second kernel in a fixed order: no atomics, the same inputs give the same bits).
   dim must be 64, batch >= 1, every pointer non-null and 16-byte aligned: FS_ERR_ARG otherwise, before any HIP call.
   fs_conv16_work_bytes returns 0 for arguments the kernels do not serve.  stream: hipStream_t. */
size_t fs_conv16_work_bytes(int batch, int dim);
int fs_conv16_forward(const float *d_x, const float *d_w, int transposed, int batch, int dim, float *d_y, void *stream);
int fs_conv16_wgrad(const float *d_x, const float *d_g, int batch, int dim, float *d_dw, void *d_work, void *stream);

/* ---- value network training: BatchNorm2d(16) on batch statistics with its activation and residual add, forward and backward
   (csrc/fs_bntrain.hip, nets.BatchNormAct16Function).  fp32, NCHW-contiguous device tensors [batch][16][64][64]; per channel
   N = batch * 4096; d_gamma, d_beta, d_save_*, d_running_*, d_dgamma, d_dbeta are device float32 [16].
     fs_bn16_forward    mean_c = sum x / N, var_c = sum (x - mean_c)^2 / N (biased), invstd_c = 1 / sqrt(var_c + eps),
                        z = (x - mean_c) * invstd_c * gamma_c + beta_c (+ d_residual when it is given),
                        d_y = z > 0 ? z : slope * z        (slope 0: ReLU, 0.01: LeakyReLU, 1: no activation).
                        Writes d_save_mean = mean, d_save_invstd = invstd.  When d_running_mean and d_running_var are given
                        (both or neither) they are updated IN PLACE: running_mean <- (1 - momentum) running_mean + momentum mean,
                        running_var <- (1 - momentum) running_var + momentum var N / (N - 1).  The statistics are accumulated in
                        float64 about each plane's first element and merged as (mean, M2) groups: a channel whose mean is large
                        against its spread keeps its variance, a constant channel has variance exactly 0.
     fs_bn16_backward   dz = d_dy * (d_y > 0 ? 1 : slope): the mask is that of the STORED forward output d_y, it is never
                        recomputed from d_x (slope 1: d_y is not read).  d_dbeta_c = sum dz, d_dgamma_c = sum dz * xh with
                        xh = (x - mean_c) * invstd_c, d_dx = gamma_c * invstd_c * (dz - dbeta_c / N - xh * dgamma_c / N),
                        d_dresidual = dz when it is given (null: no residual was given to the forward).
   d_work: fs_bn16_work_bytes(batch, 64) bytes of device scratch (per-plane partial sums; the apply kernels add them in a fixed
   order).  No atomics and no arrival counters: the same inputs give the same bits.  Not in place: d_y != d_x, d_dx != d_dy.
   dim must be 64, batch >= 1, every required pointer non-null, every given pointer 16-byte aligned, the running pointers both
   given or both null: FS_ERR_ARG otherwise, before any HIP call.  fs_bn16_work_bytes returns 0 for arguments the kernels do not
   serve.  stream: hipStream_t. */
size_t fs_bn16_work_bytes(int batch, int dim);
int fs_bn16_forward(const float *d_x, const float *d_residual, const float *d_gamma, const float *d_beta, float eps, float slope,
                    float momentum, float *d_running_mean, float *d_running_var, int batch, int dim, float *d_y, float *d_save_mean,
                    float *d_save_invstd, void *d_work, void *stream);
int fs_bn16_backward(const float *d_x, const float *d_y, const float *d_dy, const float *d_gamma, const float *d_save_mean,
                     const float *d_save_invstd, float slope, int batch, int dim, float *d_dx, float *d_dresidual, float *d_dgamma,
                     float *d_dbeta, void *d_work, void *stream);

/* ---- value network training: the first layer, the last layer at one pixel per sample, and Adam (csrc/fs_edgetrain.hip,
   nets.ConvInFunction, nets.HeadPixelFunction, train.HipAdam).  fp32, NCHW-contiguous device tensors of 64 x 64 maps.
     fs_convin_forward   d_y [batch][16][64][64] = conv3x3(d_x [batch][channels][64][64], W), stride 1, zero padding 1, no bias;
                         channels is 1, 3 or 4 and d_w the layer's weight on the device in PyTorch's layout [16][channels][3][3].
                         An image's result does not depend on the batch it is in (bit for bit).
     fs_convin_wgrad     d_dw[oc][ic][ky][kx] = sum over b, y, x of d_g[b][oc][y][x] * d_x[b][ic][y+ky-1][x+kx-1], terms outside the
                         image zero.  d_work: fs_convin_work_bytes(channels, batch, 64) bytes of device scratch (per-strip
                         partials, added by a second kernel in a fixed order).  There is no data gradient: d_x is the observation.
     fs_head_forward     d_pred[b] = sum over ic, ky, kx of W[0][ic][ky][kx] * d_h[b][ic][y+ky-1][x+kx-1] with (y, x) =
                         divmod(d_pix[b], 64), terms outside the image zero: the value the dense 16 -> 1 convolution has at that
                         pixel.  d_h [batch][16][64][64], d_w [1][16][3][3], d_pix int32 [batch] with values in [0, 4096) (a
                         value outside is clamped into the range, never used as it is).
     fs_head_backward    writes ALL of d_dh [batch][16][64][64]: +0 everywhere except d_dh[b][ic][y+ky-1][x+kx-1] =
                         d_gpred[b] * W[0][ic][ky][kx], clipped at the border; d_dw[0][ic][ky][kx] = sum over b, front to back, of
                         d_gpred[b] * d_h[b][ic][y+ky-1][x+kx-1].  Not in place (d_dh != d_h).
   dim must be 64, batch >= 1, channels 1, 3 or 4, every pointer non-null and 16-byte aligned: FS_ERR_ARG otherwise, before any
   HIP call.  fs_convin_work_bytes returns 0 for arguments the kernels do not serve.  No atomics and no arrival counters: the
   same inputs give the same bits.  stream: hipStream_t. */
size_t fs_convin_work_bytes(int channels, int batch, int dim);
int fs_convin_forward(const float *d_x, const float *d_w, int channels, int batch, int dim, float *d_y, void *stream);
int fs_convin_wgrad(const float *d_x, const float *d_g, int channels, int batch, int dim, float *d_dw, void *d_work, void *stream);
int fs_head_forward(const float *d_h, const float *d_w, const int *d_pix, int batch, int dim, float *d_pred, void *stream);
int fs_head_backward(const float *d_h, const float *d_w, const int *d_pix, const float *d_gpred, int batch, int dim, float *d_dh,
                     float *d_dw, void *stream);

/* ---- value network training: the last layer at MANY pixels per image (csrc/fs_edgetrain.hip, trainops.HeadPixelsFunction): one
   image of a measured reward map carries K labelled pixels, and the update wants one forward of the image, the last layer at
   those K pixels and one backward.
     d_h [batch][16][64][64], d_w [1][16][3][3]; d_offsets int32 [batch + 1] in CSR form -- image b owns list entries
     [d_offsets[b], d_offsets[b + 1]), possibly none; d_pix int32 [n_pixels], flat pixels in [0, 4096).
     fs_head_forward_pixels   d_pred[l] = sum over ic, ky, kx of W[0][ic][ky][kx] * d_h[b(l)][ic][y+ky-1][x+kx-1] with (y, x) =
                              divmod(d_pix[l], 64) and b(l) the image that owns entry l, terms outside the image zero: the value
                              the dense 16 -> 1 convolution has there.  Term for term the sum of fs_head_forward: with one
                              pixel per image the two give the same bits.
     fs_head_backward_pixels  writes ALL of d_dh [batch][16][64][64]: d_dh[b][ic][y][x] = the sum over the listed pixels q of image
                              b whose 3 x 3 patch covers (y, x) of d_gpred[q] * W[0][ic][ky][kx], (ky, kx) the tap of q that lies
                              on (y, x); +0 elsewhere, every plane of an image without entries included.  The order of that sum:
                              the nine taps ky = 0, 1, 2 and within each kx = 0, 1, 2, over a gradient plane that holds
                              d_gpred[q] at q and 0 at unlisted pixels (a tap without a listed pixel adds a zero).
                              d_dw[0][ic][ky][kx] = sum over all list entries l of d_gpred[l] * d_h[b(l)][ic][y+ky-1][x+kx-1].
                              The order of that sum is a fixed tree: chunk c = entries [64 c, 64 c + 64) of the list (which runs
                              per image in list order, images front to back) is added front to back; chunk sums c, c + 16,
                              c + 32, ... are added front to back into sixteen slices; the sixteen slices are added pairwise
                              ((0 + 1) + (2 + 3)) + ...  d_work: fs_head_pixels_work_bytes(batch, n_pixels, 64) bytes of device
                              scratch (the chunk sums).  Not in place (d_dh != d_h).
   Precondition: the pixels of ONE image are distinct (two images may list the same pixel) -- the caller's to guarantee
   (trainops.check_pixel_table); with a repeated pixel one of its gradients is lost from d_dh.  Every value read from d_offsets
   and d_pix is clamped into its range before it is used: a bad table gives wrong numbers, never a bad address.
   No atomics and no arrival counters: equal inputs give equal bits, and an image's d_pred and d_dh do not depend on what else is
   in the batch.  dim must be 64, batch >= 1, n_pixels >= 1, every pointer non-null and 16-byte aligned, d_dh != d_h: FS_ERR_ARG
   otherwise, with a message, before any HIP call.  fs_head_pixels_work_bytes returns 0 for arguments the kernels do not serve.
   stream: hipStream_t. */
size_t fs_head_pixels_work_bytes(int batch, int n_pixels, int dim);
int fs_head_forward_pixels(const float *d_h, const float *d_w, const int *d_offsets, const int *d_pix, int batch, int n_pixels,
                           int dim, float *d_pred, void *stream);
int fs_head_backward_pixels(const float *d_h, const float *d_w, const int *d_offsets, const int *d_pix, const float *d_gpred,
                            int batch, int n_pixels, int dim, float *d_dh, float *d_dw, void *d_work, void *stream);

/*   fs_adam_step        torch.optim.Adam's update (no amsgrad, weight decay added to the gradient) of every segment of a HOST
                         table, in fp32:  g' = g + weight_decay p;  m += (g' - m)(1 - beta1);  v = beta2 v + (1 - beta2) g' g';
                         p -= (lr / bias_correction1) * m / (sqrt(v) / sqrt(bias_correction2) + eps).
                         The bias corrections 1 - beta^t are formed by the caller in double.  A segment is four device float
                         pointers (4-byte aligned; param, exp_avg, exp_avg_sq are updated in place, grad is read) and a count of
                         elements.  The table travels as a kernel argument: one launch per 80 segments, no copy, no host
                         synchronisation.  FS_ERR_ARG before any HIP call for a null table, n_segments < 1, a segment with a null
                         or misaligned pointer or count < 1, a negative lr / eps / weight_decay, a beta outside [0, 1) or a bias
                         correction outside (0, 1]. */
typedef struct fs_adam_segment {
    void *param;
    const void *grad;
    void *exp_avg;
    void *exp_avg_sq;
    long long count;
} fs_adam_segment;
int fs_adam_step(const fs_adam_segment *segments, int n_segments, double lr, double beta1, double beta2, double eps,
                 double weight_decay, double bias_correction1, double bias_correction2, void *stream);

/* ---- training batches out of a device-resident replay buffer (flingbot_amd/replay.py) ------------------------------
   GraspDataset.__getitem__ (learning/utils.py:76-100) for a whole batch in ONE launch, one workgroup per sample:
     d_obs float32 [n_samples][4][64][64], d_masks bytes [n_samples][64][64] (0 / 1), d_labels float32 [n_samples]: the set;
     d_table int32 [batch][9] on the device: sample index, the four jitter operations in the order they run
       (0 brightness, 1 contrast, 2 saturation, 3 hue: torchvision's numbering), the bits of the four float32 factors
       indexed by operation;
     channels channel_offset .. channel_offset + channels - 1 of each drawn observation go to d_out_obs
       [batch][channels][64][64]; the mask to d_out_mask [batch][64][64]; the label to d_out_label [batch].
   jitter = 0: the recorded floats are copied unchanged.  jitter = 1 (channel_offset 0, channels 3 only): quantise with
   trunc(clamp(x * 255, 0, 255)), run torchvision's ColorJitter chain for PIL inputs bit for bit as Pillow computes it
   (csrc/fs_replay.hip has the statements), divide by 255.  A table row whose index is outside [0, n_samples) reads
   nothing and leaves its outputs unwritten.  size must be 64 and the buffers 16-byte aligned (FS_ERR_ARG otherwise). */
int fs_replay_sample(const float *d_obs, const unsigned char *d_masks, const float *d_labels, int n_samples,
                     const int *d_table, int batch, int channel_offset, int channels, int jitter, int size,
                     float *d_out_obs, unsigned char *d_out_mask, float *d_out_label, void *stream);

/* ---- the training loss with a pairwise ranking term over groups (csrc/fs_grouploss.hip, trainops.GroupLossFunction) ----
   Value AND gradient of
       loss = mse + weight * rank,    mse = (1/batch) sum_i (p_i - y_i)^2,    rank = (1/P) sum_pairs softplus(-(p_i - p_j) / temperature)
   in ONE launch of one workgroup.  d_pred, d_label: float32 [batch]; d_bounds: int32 [batch][2], row i the [begin, end) of the
   SEGMENT of the batch that sample i belongs to (replay.ExperienceSet.draw_groups: the lanes of one observation lie side by
   side).  The ordered pairs are the (i, j), j in i's segment, with  (double)y_i > (double)y_j + min_gap  -- evaluated in double
   exactly as written; P is their number and C the number of them with p_i > p_j (the concordant ones).  With P = 0, rank is
   +0.0f exactly.
     d_dpred[i] = grad_scale * [ 2 (p_i - y_i) / batch
                                 + weight / (P temperature) * ( sum_{j: (j, i) a pair} sigma(-(p_j - p_i) / temperature)
                                                              - sum_{j: (i, j) a pair} sigma(-(p_i - p_j) / temperature) ) ]
                  the second term ABSENT (not multiplied by zero) when P = 0 or weight = 0: the bits are then those of the
                  squared error's gradient alone;
     d_stats[8] = { loss, mse, rank, P, C, 0, 0, 0 }: P and C are exact as floats (at most 4096 * 4095 / 2 < 2^24 pairs).
   softplus(x) = max(x, 0) + log1p(exp(-|x|)) and sigma(x) from exp(-|x|): |p_i - p_j| / temperature of 1e4 and beyond gives
   finite results.  x is formed in double and exp(-|x|) = expf(-head) * (1 - tail) for its float head and tail, so the error
   of an addend does not grow with |x|.  A NaN prediction or label joins no pair through its own comparison (comparisons with
   NaN are false) and makes loss and mse NaN through the squared error, as torch's mse_loss does.
   Every begin / end read is clamped into [0, batch] and into begin <= end: a malformed table gives wrong numbers, never an
   access outside the batch.  Fixed-order reductions (64-lane shuffle, then LDS), no atomics: equal inputs give equal bits.
   FS_ERR_ARG with a message, before any HIP call, for: a null or non-4-byte-aligned pointer, batch
   outside 1 .. 4096, weight < 0, temperature <= 0, min_gap < 0, or any of weight / temperature / min_gap / grad_scale (or
   1 / temperature) not finite.  stream: hipStream_t.  Cost on an MI355X: 13 us at batch 128 in segments of 4; the work grows
   with the sum of the squared segment lengths on ONE compute unit -- 14.7 ms for a single segment of 4096 samples. */
int fs_group_loss(const float *d_pred, const float *d_label, const int *d_bounds, int batch, double weight, double temperature,
                  double min_gap, double grad_scale, float *d_dpred, float *d_stats, void *stream);

/* ---- the same loss over IMAGES with many labels each (csrc/fs_maploss.hip, trainops.MapLossFunction) -------------------
   fs_group_loss' rule with one segment per image, for any number of images and any total number of labels, normalised per
   label or per image.  d_pred, d_label: float32 [labels]; d_offsets: int32 [images + 1] in the CSR form of
   fs_head_forward_pixels: image b owns entries [off[b], off[b + 1]), K_b of them, possibly none.  The ordered pairs of image b
   are the (i, j), both in b, with  (double)y_i > (double)y_j + min_gap  -- evaluated in double exactly as written; P_b is their
   number and C_b the number of them with p_i > p_j.  With
       S_b = sum_{i in b} (p_i - y_i)^2,    R_b = sum_{pairs of b} softplus(-(p_i - p_j) / temperature),
       g_i = sum_{j: (j, i) a pair} sigma(-(p_j - p_i) / temperature) - sum_{j: (i, j) a pair} sigma(-(p_i - p_j) / temperature),
       L = labels,  P = sum_b P_b,  C = sum_b C_b,  G' = the images with K_b > 0,  G'' = the images with P_b > 0:
     per_image = 0 (the mean over labels, fs_group_loss' formula):
       mse = (sum_b S_b) / L,    rank = (sum_b R_b) / P,
       d_dpred[i] = grad_scale * [ 2 (p_i - y_i) / L  +  weight / (P temperature) * g_i ]
     per_image = 1 (the mean over images of the image's mean):
       mse = (1/G') sum_b S_b / K_b,    rank = (1/G'') sum_{b: P_b > 0} R_b / P_b,
       d_dpred[i] = grad_scale * [ 2 (p_i - y_i) / (G' K_b)  +  weight / (G'' P_b temperature) * g_i ],  b the image of i;
     loss = mse + weight * rank in both.  rank is +0.0 exactly when P = 0.  The second term of d_dpred is ABSENT (not multiplied
     by zero) for an image without pairs and everywhere when weight = 0; the first is the expression
     2.0f * (p - y) / (float)L of fs_group_loss, so with weight = 0 or P = 0 and per_image = 0 d_dpred has the bits fs_group_loss
     writes for the same predictions and labels;
     d_stats[8] (DOUBLE) = { loss, mse, rank, P, C, G', G'', 0 }: P passes 2^24 once the batch is not capped;
     d_table float32 [images][4], row b = { S_b / K_b, R_b / P_b (+0.0 without pairs), P_b, C_b }, all +0.0 for an empty image;
       P_b and C_b are exact as floats (at most 4096 * 4095 / 2 < 2^24 pairs in an image).
   softplus, sigma, the double x with its float head and tail, and NaN (joins no pair, reaches loss, mse and its image's
   S_b / K_b through the squared error) are fs_group_loss', from the same code (csrc/fs_pair_terms.h).
   Two launches.  The first runs a grid of (image, chunk of 256 samples): a workgroup holds its image's (p, y) in LDS and every
   thread walks the image for one sample, so a long image is spread over up to 16 compute units; g_i and the chunk sums go to
   d_work (fs_map_loss_work_bytes(images, labels) bytes of device scratch, 8-byte aligned; 0 for arguments the kernels do not
   serve).  The second forms the totals and writes d_dpred, d_stats and d_table.  Reduction order: within a chunk 64-lane
   shuffle, then the 4 wave sums front to back; the chunks of an image front to back in fp32; the images in double, image b on
   thread b mod 256, then shuffle and wave sums as before.  No atomics and no arrival counters: equal inputs give equal bits,
   and S_b, R_b, P_b, C_b and g_i have the same bits wherever the image sits in the batch and whatever else the batch holds --
   the other images enter d_dpred only through L, P, G' and G''.
   Every offset read is clamped:  begin = clamp(off[b], 0, L),  end = clamp(off[b + 1], begin, L),  end = min(end, begin + 4096)
   -- an image serves its first 4096 labels.  A malformed table gives wrong numbers, never a bad address; a d_dpred entry that no
   clamped image owns is left unwritten (trainops.MapLossFunction refuses such tables on the host).
   FS_ERR_ARG with a message, before any HIP call, for: a null pointer, a float or int pointer that is not 4-byte aligned, d_stats
   or d_work not 8-byte aligned, images < 1, labels < 1, per_image not 0 or 1, weight < 0, temperature <= 0, min_gap < 0, or any
   of weight / temperature / min_gap / grad_scale (or 1 / temperature) not finite.  stream: hipStream_t.
   Cost on an MI355X (scripts/map_loss_timing.py, EXPERIMENTS R26.1; both launches, back to back): 1.74 ms for one image of 4096
   labels, where fs_group_loss takes 14.7 ms; 0.070 ms at 28 images x 144 labels, where it takes 0.52 ms. */
size_t fs_map_loss_work_bytes(int images, int labels);
int fs_map_loss(const float *d_pred, const float *d_label, const int *d_offsets, int images, int labels, double weight,
                double temperature, double min_gap, int per_image, double grad_scale, float *d_dpred, double *d_stats,
                float *d_table, void *d_work, void *stream);

/* ---- the LISTWISE term over the same images (csrc/fs_maplist.hip, trainops.MapListFunction) ----------------------------
   Per image the KL divergence between the Boltzmann distribution of its labels and that of its predictions (ListNet's top-one
   cross-entropy), value and gradient, in O(K_b).  The operands are fs_map_loss': d_pred, d_label float32 [labels], d_offsets
   int32 [images + 1] in CSR form, image b owning K_b entries.  An image is LISTED when K_b >= 2.  For a listed image, every
   quantity formed in double from the fp32 inputs, with T_p = pred_temperature and T_y = label_temperature:
       a_i = p_i / T_p,    c_i = y_i / T_y,
       ls_i = a_i - (max a + log sum_j exp(a_j - max a)),    lq_i likewise from c,        s_i = exp(ls_i),  q_i = exp(lq_i),
       D_b = sum_i q_i (lq_i - ls_i)  = KL(q || s) >= 0,     g_i = (s_i - q_i) / T_p  = dD_b / dp_i.
   The log-sum is evaluated as log1p of the sum WITHOUT the arg-max's own addend (which is 1), and ls_i as (a_i - max a) minus
   that: no cancellation and no overflow, and a spread of 10^4 temperatures gives finite ls_i; an addend of D_b whose q_i has
   underflowed to 0 is exactly 0.  D_b is convex in p, and with T_p = T_y it is 0 exactly where p - y is constant over the image.
   With G_l the number of listed images and L_l the sum of their K_b:
     per_image = 0:  list = sum_b K_b D_b / L_l,   coef_b = K_b / L_l      (every label weighs the same)
     per_image = 1:  list = sum_b D_b / G_l,       coef_b = 1 / G_l        (every image weighs the same)
     d_dpred[i] = (float)(grad_scale * weight * coef_b * g_i) for the labels of listed images -- one rounding to fp32 -- and 0.0f
       for the labels of images that are not listed and for every label when weight = 0; an entry no image owns is not written;
     d_stats[8] (DOUBLE) = { weight * list, list, G_l, L_l, H, chosen_mass, best_mass, 0 }: H the listed images whose arg-max of
       p is their arg-max of y; chosen_mass the mean over the listed images of q at the arg-max of p -- the share of the target
       mass the net's choice carries -- and best_mass the mean of max q, its ceiling; list and both means are 0 when G_l = 0;
     d_table float32 [images][4], row b = { D_b, q at the arg-max of p, the arg-max of p, the arg-max of y } with the indices
       counted within the image (exact: < 4096); { 0, 0, -1, -1 } for an image that is not listed.
   An arg-max is the lowest index among the largest values; a NaN never wins a comparison (an image of NaNs names index 0).
   A NaN or an infinity in an image makes that image's D_b and g -- and with them the totals -- non-finite and leaves every other
   image's d_dpred and table row bit-identical.
   Two launches.  The first runs one workgroup of 256 threads per image: thread t holds labels t, t + 256, ... as doubles in
   registers, at most 16, and an image pays only for the slots it reaches; five block reductions (two arg-max, two sums of exp,
   D_b); g_i as DOUBLE and a 32-byte record per image go to d_work (fs_map_list_work_bytes(images, labels) bytes of device
   scratch, 8-byte aligned; 0 for arguments the kernels do not serve).  The second forms G_l, L_l and the totals and writes
   d_dpred and d_stats.  Reduction order: the labels of a thread in rising index, 64-lane shuffle, then the 4 wave results front
   to back; the images in double, image b on thread b mod 256, then shuffle and wave results as before; the arg-max order is
   total, so its winner does not depend on the order.  No atomics and no arrival counters, nothing read back: equal inputs give
   equal bits, and D_b, g_i and the table row have the same bits wherever the image sits in the batch and whatever else the batch
   holds -- the other images enter d_dpred only through G_l and L_l, that is through their label counts.
   Every offset read is clamped as in fs_map_loss:  begin = clamp(off[b], 0, L),  end = clamp(off[b + 1], begin, L),  end =
   min(end, begin + 4096).  A malformed table gives wrong numbers, never a bad address (trainops.MapListFunction refuses such
   tables on the host).
   FS_ERR_ARG with a message, before any HIP call, for: a null pointer, a float or int pointer that is not 4-byte aligned, d_stats
   or d_work not 8-byte aligned, images < 1, labels < 1, per_image not 0 or 1, weight < 0, a temperature <= 0, or any of weight /
   the temperatures / their reciprocals / grad_scale not finite, as doubles or as floats.  stream: hipStream_t.
   Cost on an MI355X (scripts/map_list_timing.py, EXPERIMENTS R31.1; both launches, back to back): 0.022 ms for one image of 4096
   labels and 0.019 ms at 32 and at 1000 images x 144 labels -- the host's enqueue, the kernels hide behind it -- where fs_map_loss
   takes 1.73, 0.069 and 0.131 ms. */
size_t fs_map_list_work_bytes(int images, int labels);
int fs_map_list_loss(const float *d_pred, const float *d_label, const int *d_offsets, int images, int labels, double weight,
                     double pred_temperature, double label_temperature, int per_image, double grad_scale, float *d_dpred,
                     double *d_stats, float *d_table, void *d_work, void *stream);

/* ---- the listwise term as a function of the prediction temperature (csrc/fs_mapsweep.hip, trainops.map_list_sweep) --------
   fs_map_list_loss' D_b for up to 64 prediction temperatures at once, with its first and second derivative in beta = 1 / T_p and
   what a Boltzmann policy at each temperature earns on the recorded cells: what trainops.fit_temperature minimises, in ONE pass
   over the labels.  The operands are fs_map_list_loss': d_pred, d_label float32 [labels], d_offsets int32 [images + 1] in CSR
   form, image b owning K_b entries, LISTED when K_b >= 2.  `temperatures` is a HOST array of n_temperatures doubles (1 to 64; it
   is read before the call returns and travels as kernel arguments).  For a listed image, every quantity formed in double from the
   fp32 inputs, with T_y = label_temperature, beta_s = 1 / temperatures[s], m the arg-max of p and d_i = p_i - p_m:
       c_i = y_i / T_y,   lq_i = c_i - (max c + log sum_j exp(c_j - max c)),   q_i = exp(lq_i)            (fs_map_list_loss' q)
       e_i = exp(beta_s d_i),   Z' = sum_{i != m} e_i,   s_i = e_i / (1 + Z')  = softmax(beta_s p)_i,
       D_b(beta_s)   = sum_i q_i lq_i  -  beta_s sum_i q_i d_i  +  (sum_i q_i) log1p(Z')      = sum_i q_i (lq_i - ls_i) = KL(q || s),
       dD_b/dbeta    = E_s[p] - E_q[p]    = sum_i s_i d_i - sum_i q_i d_i,
       d2D_b/dbeta2  = Var_s[p] >= 0      = max(sum_i s_i d_i^2 - (sum_i s_i d_i)^2, 0):  D_b is convex in beta.
   The log-sum is log1p of the sum WITHOUT the arg-max's own addend (which is 1); an addend of the three q-sums whose q_i has
   underflowed to 0 is exactly 0; sum_i q_i is 1 up to rounding and is kept, so D_b is the sum fs_map_list_loss forms.  The
   moments are taken about p_m, and E_s[y] about max y: no cancellation at a low temperature, where s sits on the arg-max.
     d_rows   double [images][n_temperatures][4], row (b, s) = { D_b(beta_s), E_s[p] - E_q[p], Var_s[p], E_s[y] }; zeros for an
              image that is not listed;
     d_images double [images][4], row b = { K_b, y at the arg-max of y, y at the arg-max of p, E_q[p] = p_m + sum_i q_i d_i };
              { 0, 0, 0, 0 } for an image that is not listed;
     d_curve  double [n_temperatures][8], row s = { list, slope, curvature, expected_regret, best_draw, greedy_draw, G_l, L_l }:
              list = sum_b coef_b D_b(beta_s) with fs_map_list_loss' coef_b (K_b / L_l for per_image = 0, 1 / G_l for 1) -- its
              d_stats[1] at pred_temperature = temperatures[s]; slope and curvature the same sums of the two derivatives;
              expected_regret the mean over the listed images of  y at the arg-max of y  -  E_s[y],  best_draw that of s at the
              arg-max of y and greedy_draw that of s at the arg-max of p: what drawing a cell with probability s earns, how often
              it draws the best cell, and how often the net's own choice.  The first six are 0 when G_l = 0.
   An arg-max is the lowest index among the largest values; a NaN never wins a comparison.  A NaN or an infinity in an image
   makes every entry of that image's d_rows rows (the sum of x - x over its values, 0 or NaN, is added to each) and with them
   columns 0-5 of every d_curve row non-finite, and leaves every other image's d_rows and d_images rows bit-identical.
   Two launches.  The first runs one workgroup of 256 threads per image: thread t holds labels t, t + 256, ... as doubles in
   registers, at most 16; the arg-maxes, q and the three q-sums are formed once, then the temperatures are walked with the labels
   still in registers, ONE block reduction each that carries Z', sum e d, sum e d^2 and sum e (y - max y) together; s at the two
   arg-maxes is 1 / (1 + Z') and exp(beta_s d at the arg-max of y) / (1 + Z').  Those two per image and temperature go to d_work
   (fs_map_list_sweep_work_bytes(images, labels, n_temperatures) bytes of device scratch, 8-byte aligned; 0 for arguments the
   kernels do not serve).  The second runs one workgroup per temperature and reduces the images to d_curve.  Reduction order:
   the labels of a thread in rising index, 64-lane shuffle, then the 4 wave results front to back; the images in double, image b
   on thread b mod 256, then shuffle and wave results as before.  No atomics and no arrival counters, nothing read back: equal
   inputs give equal bits, and an image's d_rows and d_images rows have the same bits wherever the image sits in the batch and
   whatever else the batch holds.
   Every offset read is clamped as in fs_map_list_loss:  begin = clamp(off[b], 0, L),  end = clamp(off[b + 1], begin, L),  end =
   min(end, begin + 4096).  A malformed table gives wrong numbers, never a bad address (trainops.map_list_sweep refuses such
   tables on the host).
   FS_ERR_ARG with a message, before any HIP call, for: a null pointer, a float or int pointer that is not 4-byte aligned,
   temperatures / d_curve / d_rows / d_images / d_work not 8-byte aligned, images < 1, labels < 1, n_temperatures outside 1..64,
   per_image not 0 or 1, and any temperature, label_temperature or one of their reciprocals that is not positive and finite, as
   a double or as a float.  stream: hipStream_t.
   Cost on an MI355X (scripts/map_sweep_timing.py, EXPERIMENTS R32.1; both launches, back to back), 33 / 64 temperatures: 0.047 /
   0.081 ms at 32 images x 144 labels, 0.111 / 0.196 ms at 1000 x 144 and 0.088 / 0.150 ms for one image of 4096 labels, where one
   fs_map_list_loss call per temperature takes 0.62 / 1.23, 0.62 / 1.26 and 0.73 / 1.42 ms; a whole trainops.fit_temperature (six
   sweeps of 33, six downloads) 0.78 / 1.19 / 1.02 ms. */
size_t fs_map_list_sweep_work_bytes(int images, int labels, int n_temperatures);
int fs_map_list_sweep(const float *d_pred, const float *d_label, const int *d_offsets, int images, int labels,
                      const double *temperatures, int n_temperatures, double label_temperature, int per_image, double *d_curve,
                      double *d_rows, double *d_images, void *d_work, void *stream);

/* ---- the rank statistics of recorded reward maps under the current weights (csrc/fs_mapscore.hip, trainops.map_score) ---
   What probe.map_stats computes on the host for one map, for a whole batch of images in ONE launch, from the dense value maps the
   eval forward wrote.  d_value: float32 [images][value_stride] (the [B, 1, 64, 64] output: value_stride = 4096); d_pix int32
   [labels], d_label float32 [labels] and d_offsets int32 [images + 1] in the CSR form of fs_map_loss / fs_head_forward_pixels:
   image b owns list positions [off[b], off[b + 1]), at most 4096 of them, possibly none.  The prediction at position l of image b
   is  p_l = d_value[b * value_stride + pix[l]],  its label y_l = d_label[l].  A position is COUNTED when both p_l and y_l are
   finite; everything below is over the counted positions of b alone, k = the position inside the image (l - off[b]).
     d_rows double [images][12], every integer stored exactly as a double; row b =
       0  n            the number of counted positions
       1  chosen       the counted k with the largest p; among equals the lowest k
       2  best         the counted k with the largest y; among equals the lowest k
       3  chosen_rank  the number of counted positions with y > y_chosen
       4  P_b          the ordered pairs (i, j) with  (double)y_i > (double)y_j + min_gap  -- fs_map_loss' rule, evaluated in
                       double exactly as written
       5  C_b          how many of those pairs have p_i > p_j
       6  Sab          sum_i a_i b_i,   a_i = 2 #{j: p_j < p_i} + #{j: p_j == p_i} + 1 - (n + 1)  (j = i among the equal),
       7  Saa          sum_i a_i^2,     b_i the same over y: the centred doubled average ranks.  Integers of at most 7e10 in
       8  Sbb          sum_i b_i^2      magnitude, accumulated in 64-bit integers: exact
       9  spearman     (double)Sab / sqrt((double)Saa * (double)Sbb); NaN when n < 2 or Saa = 0 or Sbb = 0
      10  regret       (double)y_best - (double)y_chosen
      11  se           sum ((double)p - (double)y)^2, summed in double
     An image with n = 0 writes n = 0, columns 1-3 = -1, columns 4-8 = 0, columns 9-10 NaN and column 11 = 0.
   One workgroup of 256 threads per image: its (p, y) in LDS, the samples strided over the threads, every thread walking the
   whole image for each of its samples.  Reduction order: the samples of a thread in rising k, 64-lane shuffle, then the 4 wave
   results front to back; the arg-max reductions carry (value, k), so ties go to the lowest k whatever lane holds them.  No
   atomics, no arrival counters, no scratch: equal inputs give equal bits, and a row depends on neither the image's place in the
   batch nor on the other images.  The division and the square root of column 9 are IEEE double operations.
   Every offset read is clamped:  begin = clamp(off[b], 0, L),  end = clamp(off[b + 1], begin, L),  end = min(end, begin + 4096)
   -- an image serves its first 4096 positions -- and every pixel into [0, value_stride).  A malformed table gives wrong numbers,
   never a bad address (trainops.map_score refuses such tables on the host).
   FS_ERR_ARG with a message, before any HIP call, for: a null pointer, a float or int pointer that is not 4-byte aligned, d_rows
   not 8-byte aligned, images < 1, labels < 1, value_stride < 1, min_gap < 0 or not finite.  stream: hipStream_t.
   Cost on an MI355X (scripts/map_score_timing.py, EXPERIMENTS R27.1; through trainops.map_score, calls back to back): 0.045 ms
   at 64 and at 1000 images x 144 positions -- the host's enqueue, the kernel hides behind it -- where the host loop over
   probe.map_stats takes 8.2 ms and 114 ms; 2.69 ms for one image of 4096 positions against 17.6 ms: an image is ONE workgroup, so
   such an image keeps one compute unit busy -- splitting it as fs_map_loss does is not built. */
int fs_map_score(const float *d_value, int value_stride, const int *d_pix, const float *d_label, const int *d_offsets, int images,
                 int labels, double min_gap, double *d_rows, void *stream);

/* ---- the picture of a chosen action (flingbot_amd/report.py, csrc/fs_panels.hip) -----------------------------------
   environment/utils.py visualize_action (:369-432) for all ready episodes at once.  Stateless: the stream is the last
   argument; FS_ERR_ARG with a message before any HIP call for the arguments refused below.

   fs_value_range      per item the minimum and maximum over the FINITE values of `count` device floats -> d_out[2 k],
                       d_out[2 k + 1] on the device; (0, 0) when no value is finite; a zero extreme is +0.0.  The
                       `all_value_maps.min()` / `.max()` of visualize_action (:398) over the chosen primitive's maps.  `items`
                       is a HOST table that travels as kernel arguments (128 items per launch): no copy, no host
                       synchronisation.  One workgroup per item: the result depends on neither n_items nor the item's place.
                       Refused: a null table or output, n_items < 1, an item with a null or non-4-byte-aligned pointer or
                       count < 1. */
typedef struct fs_range_item {
    const float *values; /* device */
    long long count;
} fs_range_item;
int fs_value_range(const fs_range_item *items, int n_items, float *d_out, void *stream);

/* fs_action_panels    one uint8 strip [panel][5 panel][3] (rows top-down, RGB) per action into d_out [n_actions][panel]
                       [5 panel][3]:  before | value map | transformed RGB + action | before + action | after.
                       `table` is a HOST array of records; the call checks it, copies it into d_work
                       (fs_action_panels_work_bytes(n_actions) device bytes, 16-byte aligned; one upload, which waits for the
                       stream) and composes all strips in ONE launch.  A record: device pointers to the chosen stack entry
                       float32 [4][D][D], the chosen value map [D][D], the action's (vmin, vmax), the observation before and
                       after the action float32 [>= 3][S][S] (after may be null: the panel is black), and up to
                       FS_PANEL_MAX_PRIMS overlay primitives for the D x D panel (`small`) and for the S x S panel (`large`).
                       A primitive is nine ints {kind, y0, x0, y1, x1, t, r, g, b} in SOURCE pixels (row, column).
   The rules -- integer or single-rounded fp32, so that a restatement in numpy gives the same bytes:
     float -> uint8    trunc(clamp(x * 255, 0, 255)) in fp32.
     sampling          a panel shows its source by nearest sampling, source index = (dst * src_size) / panel in integer
                       division per axis; overlays are drawn at the source's resolution and sampled with it.  The RGB panels are
                       planes 0 .. 2 of their source as [row][column][channel].
     value colour      t = (v - vmin) / (vmax - vmin): fp32 subtractions, the correctly rounded fp32 quotient;
                       index = min(255, max(0, (int)(t * 256.0f))), 0 when vmax == vmin or v is not finite (or t is NaN);
                       colour = entry `index` of matplotlib's jet as 256 x 3 bytes (fs_jet_table; csrc/fs_jet_table.h).
     FS_PANEL_RING     centre (y0, x0), radius R = y1 (x1 unused), thickness t: a pixel at squared integer distance d2 from
                       the centre is covered when (2R - t)^2 <= 4 d2 <= (2R + t)^2.
     FS_PANEL_SEGMENT  from a = (y0, x0) to b = (y1, x1), v = b - a, w = p - a, L = v.v:  w.v <= 0: covered when
                       4 |w|^2 <= t^2;  w.v >= L: when 4 |p - b|^2 <= t^2;  else when 4 (w x v)^2 <= t^2 L.  int64 throughout.
     blend             a later primitive overwrites an earlier one; the covered pixel is blended once,
                       (9 * colour + base + 5) / 10 per channel in integer division (imshow(action, alpha = 0.9)).
   Coordinates may lie outside the image; only pixels inside are tested.  A strip is a function of its own record alone.
   Refused: a null table / d_out / d_work, n_actions outside 1 .. 65535, D (obs_dim), S (image_dim) or panel outside 1 .. 4096,
   a misaligned buffer, a record with a null stack / value map / range / before pointer, more than 8 primitives on a panel,
   an unknown kind, |coordinate| > 8191, t outside 1 .. 64, a colour outside 0 .. 255.
   fs_jet_table        the compiled-in colour table, 768 bytes (host only). */
#define FS_PANEL_RING 0
#define FS_PANEL_SEGMENT 1
#define FS_PANEL_MAX_PRIMS 8
typedef struct fs_panel_record {
    const float *stack;
    const float *value_map;
    const float *range;
    const float *before;
    const float *after;
    int n_small, n_large;
    int small[FS_PANEL_MAX_PRIMS][9];
    int large[FS_PANEL_MAX_PRIMS][9];
} fs_panel_record;
size_t fs_action_panels_work_bytes(int n_actions);
int fs_action_panels(const fs_panel_record *table, int n_actions, int obs_dim, int image_dim, int panel, unsigned char *d_out,
                     void *d_work, void *stream);
int fs_jet_table(unsigned char *out, int n_bytes);

/* fs_lane_panels      the picture of a look-ahead step (flingbot_amd/lookahead.py): one uint8 strip [panel][(1 + lanes) panel][3]
                       per record into d_out [n_records][panel][(1 + lanes) panel][3].  Panel 0 is the observation before the
                       step with the action of EVERY executed lane drawn on it; panel 1 + j is the observation after lane j.
                       `table` is a HOST array of records; the call checks it, copies it into d_work
                       (fs_lane_panels_work_bytes(n_records) device bytes, 16-byte aligned; one upload, which waits for the
                       stream) and composes all strips in ONE launch.  A record: the device pointers `before` and `after[j]`,
                       float32 [>= 3][S][S]; n_lanes executed lanes (1 .. lanes); `followed`, the lane the episode continued
                       from (-1: none); per lane n_prims[j] <= FS_PANEL_MAX_PRIMS primitives {kind, y0, x0, y1, x1, t, r, g, b}
                       in SOURCE pixels, as for fs_action_panels.
   The rules are fs_action_panels' -- float -> uint8, nearest sampling (dst * S) / panel with the overlays drawn at the source's
   resolution, ring and segment coverage, one blend (9 * colour + base + 5) / 10 -- and these:
     rank colours      every primitive of lane j is drawn in entry j of a fixed table (fs_lane_colours), whatever r, g, b it
                       carries (they are still checked):  0 (230, 25, 75)  1 (60, 180, 75)  2 (0, 130, 200)  3 (245, 130, 48)
                       4 (145, 30, 180)  5 (70, 240, 240)  6 (240, 50, 230)  7 (255, 225, 25).
     order             lanes are drawn in rank order and a later primitive overwrites an earlier one, across lanes too: a pixel
                       of panel 0 that primitives of several lanes cover is blended once, with the colour of the HIGHEST such lane.
     frame             after the sampling, destination pixel (y, x) of an after panel, m = min(y, x, panel - 1 - y, panel - 1 - x),
                       t = max(1, panel / 50) in integer division:  m < t: the lane's rank colour;  t <= m < 2 t on the followed
                       lane's panel: white (255, 255, 255).  The frame overwrites, it does not blend.
     black             the panel of a lane j >= n_lanes, or of one whose after[j] is null, is black and has no frame (its
                       primitives, for j < n_lanes, are still on panel 0).
   A strip is a function of its own record alone.  Refused: a null table / d_out / d_work, n_records outside 1 .. 65535, lanes
   outside 1 .. FS_LANE_MAX, S (image_dim) or panel outside 1 .. 4096, a misaligned buffer, a record with a null before pointer,
   n_lanes outside 1 .. lanes, followed outside -1 .. n_lanes - 1, a pointer off the float grid, and on a lane below n_lanes
   more than 8 (or fewer than 0) primitives, an unknown kind, |coordinate| > 8191, t outside 1 .. 64, a colour outside 0 .. 255.
   fs_lane_colours     the compiled-in rank colours, 24 bytes (host only). */
#define FS_LANE_MAX 8
typedef struct fs_lane_record {
    const float *before;
    const float *after[FS_LANE_MAX];
    int n_lanes, followed;
    int n_prims[FS_LANE_MAX];
    int prims[FS_LANE_MAX][FS_PANEL_MAX_PRIMS][9];
} fs_lane_record;
size_t fs_lane_panels_work_bytes(int n_records);
int fs_lane_panels(const fs_lane_record *table, int n_records, int lanes, int image_dim, int panel, unsigned char *d_out,
                   void *d_work, void *stream);
int fs_lane_colours(unsigned char *out, int n_bytes);

/* fs_probe_panels     the picture of a probed map (flingbot_amd/probe.py): one uint8 strip [panel][4 panel][3] per record into
                       d_out [n_records][panel][4 panel][3]:  what the net saw + the chosen action | the predicted map | the
                       measured map | the observation after the best-measured cell.  `table` is a HOST array of records; the
                       call checks it, copies it into d_work (fs_probe_panels_work_bytes(n_records) device bytes, 16-byte
                       aligned; one upload, which waits for the stream) and composes all strips in ONE launch.  A record: device
                       pointers to the chosen stack entry float32 [4][D][D], the chosen value map [D][D], (vmin, vmax), the
                       measured rewards float32 [gy][gz] (NaN: not executed), the lattice's codes uint8 [gy][gz] (bit 0: valid,
                       fs_lattice_actions' code_out) and the observation float32 [>= 3][S][S] after the best cell's lane (may
                       be null); the lattice (y0, z0, stride, gy, gz) of fs_lattice_actions; the chosen cell (cy, cz), -1: none;
                       up to FS_PANEL_MAX_PRIMS primitives for the D x D panel.
   The rules are fs_action_panels' -- float -> uint8, nearest sampling (dst * src_size) / panel, the value colour, ring and
   segment coverage, one blend -- and these:
     panel 0           fs_action_panels' panel 2: planes 0 .. 2 of the stack entry with `small` drawn on them.
     panel 1           fs_action_panels' panel 1: the value map under jet over (vmin, vmax).
     panel 2           destination pixel -> map pixel (y, z) by the nearest sampling with src_size = D, then, in integer
                       division, ny = y - y0 + stride / 2, nz = z - z0 + stride / 2, cell i = ny / stride, j = nz / stride:
                         ny < 0, nz < 0, i >= gy or j >= gz              black (outside the lattice)
                         (i, j) the chosen cell and ny - i stride or nz - j stride is 0 or stride - 1      white (255, 255, 255):
                                                                         the outermost source pixels of the chosen cell
                         measured[i][j] finite                           the value colour of measured[i][j] over the SAME
                                                                         (vmin, vmax)
                         else bit 0 of code[i][j] set                    (128, 128, 128): valid, not executed
                         else                                            (64, 64, 64): invalid
     panel 3           planes 0 .. 2 of `after`; black when it is null.
   A strip is a function of its own record alone.  Refused: a null table / d_out / d_work, n_records outside 1 .. 65535, D
   (obs_dim), S (image_dim) or panel outside 1 .. 4096, a misaligned buffer, a record with a null stack / value map / range /
   measured / code pointer or a float pointer off the float grid, stride < 1, gy gz outside 1 .. 4096, a lattice that leaves
   [0, D), a chosen cell outside -1 .. gy - 1 / gz - 1, more than 8 primitives, an unknown kind, |coordinate| > 8191, t outside
   1 .. 64, a colour outside 0 .. 255. */
typedef struct fs_probe_record {
    const float *stack;
    const float *value_map;
    const float *range;
    const float *measured;
    const unsigned char *code;
    const float *after;
    int y0, z0, stride, gy, gz, cy, cz;
    int n_small;
    int small[FS_PANEL_MAX_PRIMS][9];
} fs_probe_record;
size_t fs_probe_panels_work_bytes(int n_records);
int fs_probe_panels(const fs_probe_record *table, int n_records, int obs_dim, int image_dim, int panel, unsigned char *d_out,
                    void *d_work, void *stream);

/* ---- host-only entry points (no HIP device needed) ------------------------------------------------------------
   Scene builder exposed on its own so host logic can be checked without a GPU: same arguments as fs_set_scene. */
typedef struct fs_host_scene fs_host_scene;
#define FS_SCENE_POSITIONS 0        /* float[4N] */
#define FS_SCENE_VELOCITIES 1       /* float[3N] */
#define FS_SCENE_PHASES 2           /* int[N] */
#define FS_SCENE_SPRINGS 3          /* int[2M]   (pyflex.get_edges) */
#define FS_SCENE_SPRING_LENGTHS 4   /* float[M] */
#define FS_SCENE_SPRING_STIFFNESS 5 /* float[M] */
#define FS_SCENE_TRIANGLES 6        /* int[3T]   (pyflex.get_faces) */
#define FS_SCENE_TRI_NORMALS 7      /* float[3T] */
#define FS_SCENE_ADJ_OFFSETS 8      /* int[N+1]  particle -> spring CSR */
#define FS_SCENE_ADJ_NEIGHBORS 9    /* int[2M] */
#define FS_SCENE_BOUNDS 10          /* float[6] lower, upper */
#define FS_SCENE_PARAMS 11          /* float[32] packed parameter table */
/* derived tables of the kernels (white box for the CPU tests; empty when the cloth does not have them) */
#define FS_SCENE_RESTNEAR 12        /* uint32[8][n]: per particle up to 16 ids (16 bits each, 0xffff = none) of the particles closer
                                       than the collision radius in the rest pose (SelfCollideFilter, NvFlex.h:166) */
#define FS_SCENE_STREAM_CODES 13    /* uint32[n][4]: one byte per spring slot of the particle, 255 = none */
#define FS_SCENE_STREAM_DICT 14     /* float[entries][4]: bits(j - i), rest length, stiffness, 0 */
#define FS_SCENE_FLAGS 15           /* int[4]: restnear_ok (0 none, 1 packed ids, 2 = the sets are the 8 grid neighbours), g64_ok,
                                       gp_L_ok, gp_halvable */
/* packed adjacency of a cloth WITHOUT stream codes (fs_k_iterate_mesh).  For these two selectors fs_host_scene_copy returns the
   number of elements it copied: 0 = the cloth has no words (it has stream codes, or more than four distinct stiffnesses) */
#define FS_SCENE_MESH_WORDS 16      /* uint32[max_deg][n][2], slot-major in the order of the particle's springs (ascending spring
                                       id): j | stiffness index << 30, bits of the rest length; an empty slot is 0xffffffff, 0 */
#define FS_SCENE_MESH_STIFFNESS 17  /* float[4]: the distinct stiffnesses in order of first use by spring id (unused entries 0) */
fs_host_scene *fs_host_scene_build(const float *scene_params, int n_params, const float *verts, int n_vert_floats,
                                   const int *stretch, int n_stretch_ints, const int *bend, int n_bend_ints,
                                   const int *shear, int n_shear_ints, const int *faces, int n_face_ints);
void fs_host_scene_free(fs_host_scene *h);
int fs_host_scene_counts(const fs_host_scene *h, int *n, int *m, int *t, int *max_deg);
int fs_host_scene_copy(const fs_host_scene *h, int what, void *out, int n_elems);
/* fs_set_scene from a scene fs_host_scene_build made earlier (on any thread, without the GPU): the scene is taken out of
   `scene`, which stays valid but empty (free it with fs_host_scene_free).  Same result as fs_set_scene. */
int fs_set_scene_prebuilt(fs_ctx *ctx, int env, fs_host_scene *scene);
/* host-only: the mesh of ONE kinematic sphere exactly as fs_render rasterises it (see fs_get_sphere_mesh) */
int fs_host_sphere_mesh(float radius, const float *prev_pos3, const float *prev_quat4, float *verts, float *normals,
                        int *tris);
/* host-only: the plan fs_movep* / fs_advance* make of ONE movep (simEnv.py:739-769 + flex_utils.py:223-252), or of one piece
   of it: pickers at picker_pos[S][3] (float32), targets[S][3], resumed at loop iteration `start`, at most max_steps
   simulation steps (< 0: no cap).  Out: loop iteration reached (pass it back as `start`), simulation steps, status (0 = the
   step cap was reached, 1 = targets reached, 2 = `limit` reached), the pickers afterwards (end_pos[S][3], may be null) and
   the capture points of dump_visualizations (simEnv.py:764-768): frame k follows capture_after[k] simulation steps of this
   call (0: the state the call found) in loop iteration capture_iter[k].  Returns their number, or an error code. */
int fs_host_plan_movep(int n_pickers, const float *picker_pos, const double *targets, double speed, int limit, int min_steps,
                       double eps, int f32_targets, int start, int max_steps, int *iterations_out, int *steps_out,
                       int *status_out, int *capture_after, int *capture_iter, int capture_capacity, float *end_pos);
/* RenderScene camera / light set-up (main.cpp:1411-1438; core/maths.h:507-598): out[0:16] view, [16:32] proj,
   [32:48] lightTransform (row-major, column vectors), [48:51] lightPos, [51:54] lightDir. */
int fs_camera_matrices(const float *cam_pos3, const float *cam_angle3, int width, int height,
                       const float *scene_lower3, const float *scene_upper3, float *out54);

#ifdef __cplusplus
}
#endif
#endif
