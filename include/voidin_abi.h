/*
 * voidin_abi.h — C ABI of libvoidin_hip.so, the MI355X (gfx950) implementation of
 * voidin's GPU-driven visibility path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++ / torch
 * types.  Every entry point names the reference interface it replaces; paths are relative
 * to the reference checkout (pudnax/voidin v0.69.0).
 *
 * Conventions
 *   - every function returns VD_OK (0) or a negative VdStatus; nothing aborts or throws
 *     across the boundary (the reference panics — crates/bvh/src/blas.rs:114-116 — we do not);
 *   - `*_dev` variants take DEVICE pointers (hipMalloc'd on the ctx's device) and enqueue
 *     on the ctx's stream without synchronising (exceptions, stated at their declarations:
 *     vd_bvh_build_dev, vd_dist_step_draws_dev and the traversal entry points - which read
 *     a status word back - block); the plain variants take HOST pointers,
 *     stage through ctx-owned device buffers and return after the result is in host memory;
 *   - the caller owns every in/out buffer; device scratch belongs to the VdCtx;
 *   - a VdCtx is thread-compatible, not thread-safe (the reference's `World` is
 *     RefCell-based and single-threaded: crates/components/src/world.rs:81-84).
 */
#ifndef VOIDIN_ABI_H
#define VOIDIN_ABI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------ */
/* Data contract. All little-endian, f32/u32/i32, #[repr(C)].      */
/* ------------------------------------------------------------------------------------ */

/* D1  crates/components/src/shared.rs:67-75, shaders/shared.wgsl:53-59 — 144 B */
typedef struct VdInstance {
    float    transform[16];      /* mat4, column-major: transform[4*c + r]          */
    float    inv_transform[16];  /* mat4, column-major                              */
    uint32_t mesh;               /* MeshId                                          */
    uint32_t material;           /* MaterialId                                      */
    uint32_t junk[2];
} VdInstance;

/* D2  crates/components/src/shared.rs:29-39, shaders/shared.wgsl:43-51 — 48 B */
typedef struct VdMeshInfo {
    float    min[3];
    uint32_t index_count;
    float    max[3];
    uint32_t base_index;
    int32_t  vertex_offset;
    uint32_t bvh_index;
    uint32_t junk[2];
} VdMeshInfo;

/* D3  crates/components/src/lib.rs:99-107, shaders/shared.wgsl:69-75 — 20 B */
typedef struct VdDrawIndexedIndirect {
    uint32_t vertex_count;       /* = MeshInfo.index_count                          */
    uint32_t instance_count;     /* 1 visible, 0 culled                             */
    uint32_t base_index;
    int32_t  vertex_offset;
    uint32_t base_instance;      /* = instance index (visibility.wgsl:33 reads it)  */
} VdDrawIndexedIndirect;

/* D4  crates/components/src/camera.rs:13-27, shaders/shared.wgsl:13-24 — 320 B */
typedef struct VdCameraUniform {
    float view_position[4];
    float projection[16];
    float view[16];
    float clip_to_world[16];
    float prev_world_to_clip[16];
    float frustum[4];
    float zfar;
    float znear;
    float jitter[2];
    float prev_jitter[2];
    float _padding[2];
} VdCameraUniform;

/* D5  crates/bvh/src/blas.rs:10-17, shaders/utils/bvh.wgsl:11-16 — 32 B.
 * count > 0: leaf over triangles [left_first, left_first+count) of the reordered index
 * buffer; count == 0: interior, children at node ids left_first and left_first+1.      */
typedef struct VdBvhNode {
    float    min[3];
    uint32_t left_first;
    float    max[3];
    uint32_t count;
} VdBvhNode;

/* D6  crates/bvh/src/tlas.rs:7-14, shaders/utils/bvh.wgsl:4-9 — 32 B.
 * left_right = left | right << 16 (0 => leaf); instance_idx = u32::MAX for interior.    */
typedef struct VdTlasNode {
    float    min[3];
    uint32_t left_right;
    float    max[3];
    uint32_t instance_idx;
} VdTlasNode;

/* Extended TLAS node for more than VD_TLAS_MAX_INSTANCES instances:
 * the reference packs two 16-bit ids into left_right, so it cannot address n > 32768.
 * Same build rule, children kept as two full u32. NOT a reference layout.               */
typedef struct VdTlasNodeWide {
    float    min[3];
    uint32_t left;               /* 0 and right==0 => leaf                           */
    float    max[3];
    uint32_t right;
    uint32_t instance_idx;
    uint32_t _pad[3];
} VdTlasNodeWide;

/* Ray + hit records of the batch traversal entry point (intersections.wgsl:3-11, bvh.wgsl:18-28: one
 * ray per fragment there).  _pad0 / _pad1: ignored unless VD_OPT_TRACE_RAY_RANGE ("Ray intervals"). */
typedef struct VdRay {
    float eye[3];
    float _pad0;                 /* t_min under VD_OPT_TRACE_RAY_RANGE, else unused  */
    float dir[3];
    float _pad1;                 /* t_max under VD_OPT_TRACE_RAY_RANGE, else unused  */
} VdRay;

typedef struct VdHit {
    float    dist;               /* MAX_DIST (1e30) on miss                          */
    uint32_t hit;                /* 0 / 1                                            */
    uint32_t instance;           /* instance whose BLAS produced the closest hit     */
    uint32_t triangle;           /* mesh-local triangle slot in the reordered buffer */
} VdHit;

#define VD_MAX_DIST 1e30f
#define VD_TLAS_MAX_INSTANCES 32768u
#define VD_TLAS_WIDE_MAX_INSTANCES (1u << 24)   /* vd_tlas_build_lbvh_wide*, vd_trace_wide*: 2^25 + 1 nodes at the most */

#if defined(__cplusplus)
static_assert(sizeof(VdInstance) == 144, "Instance is 144 B (shared.rs:67-75)");
static_assert(sizeof(VdMeshInfo) == 48, "MeshInfo is 48 B (shared.rs:29-39)");
static_assert(sizeof(VdDrawIndexedIndirect) == 20, "DrawIndexedIndirect is 20 B (lib.rs:99-107)");
static_assert(sizeof(VdCameraUniform) == 320, "CameraUniform is 320 B (camera.rs:13-27)");
static_assert(sizeof(VdBvhNode) == 32, "BvhNode is 32 B (blas.rs:10-17)");
static_assert(sizeof(VdTlasNode) == 32, "TlasNode is 32 B (tlas.rs:7-14)");
static_assert(sizeof(VdTlasNodeWide) == 48, "wide TLAS node is 48 B");
static_assert(sizeof(VdRay) == 32 && sizeof(VdHit) == 16, "ray/hit records");
#else
_Static_assert(sizeof(VdInstance) == 144, "Instance is 144 B");
_Static_assert(sizeof(VdMeshInfo) == 48, "MeshInfo is 48 B");
_Static_assert(sizeof(VdDrawIndexedIndirect) == 20, "DrawIndexedIndirect is 20 B");
_Static_assert(sizeof(VdCameraUniform) == 320, "CameraUniform is 320 B");
_Static_assert(sizeof(VdBvhNode) == 32, "BvhNode is 32 B");
_Static_assert(sizeof(VdTlasNode) == 32, "TlasNode is 32 B");
_Static_assert(sizeof(VdTlasNodeWide) == 48, "wide TLAS node is 48 B");
_Static_assert(sizeof(VdRay) == 32 && sizeof(VdHit) == 16, "ray/hit records");
#endif

/* ------------------------------------------------------------------------------------ */
/* Status codes                                                                          */
/* ------------------------------------------------------------------------------------ */
typedef enum VdStatus {
    VD_OK = 0,
    VD_ERR_INVALID_ARG = -1,     /* null pointer, zero/oversized count, bad capacity     */
    VD_ERR_HIP = -2,             /* HIP runtime error; text in vd_last_error             */
    VD_ERR_DEGENERATE = -3,      /* BVH input the reference builder crashes on
                                    (all 21 split candidates rejected: blas.rs:137-140)  */
    VD_ERR_TLAS_OVERFLOW = -4,   /* n > 32768 in the 16-bit reference TLAS layout
                                    (tlas.rs:71)                                         */
    VD_ERR_NO_DEVICE = -5,       /* no gfx950 device / extension built for another arch  */
    VD_ERR_STACK_OVERFLOW = -6,  /* traversal stack exceeded (reference has no check:
                                    shaders/utils/stack.wgsl:1-20).  vd_trace*: only for a
                                    stack of more than 128 + 4 Mi entries (see there);
                                    vd_traverse_iter / vd_traverse: beyond 128           */
    VD_ERR_OOM = -7,
    VD_ERR_COMM = -8             /* RCCL: library not found, communicator or collective failed;
                                    text in vd_last_error                                  */
} VdStatus;

typedef struct VdCtx VdCtx;

/* ------------------------------------------------------------------------------------ */
/* Context                                                                               */
/* ------------------------------------------------------------------------------------ */
/* Replaces the wgpu device/queue pair the passes pull from `World`
 * (crates/app/src/app.rs:108-118). One HIP stream per ctx.                              */
int         vd_ctx_create(int device, VdCtx** out_ctx);
int         vd_ctx_destroy(VdCtx* ctx);
/* Run on a caller-owned hipStream_t (e.g. the host framework's current stream); NULL is
 * the HIP default stream.  vd_ctx_reset_stream goes back to the ctx-owned stream.       */
int         vd_ctx_set_stream(VdCtx* ctx, void* hip_stream);
int         vd_ctx_reset_stream(VdCtx* ctx);
int         vd_ctx_synchronize(VdCtx* ctx);
const char* vd_last_error(const VdCtx* ctx);
const char* vd_version(void);

/* Per-context options.  The library reads NO environment variable for these (the one it reads
 * at all is VD_RCCL_LIB, the path of the RCCL shared object: "Multi-GPU exchange" below); defaults
 * are the measured optima.  They exist for A/B measurements (tools/) and so that the
 * tests can force paths that otherwise depend on timing or size (the single-workgroup redo of the
 * TLAS chain, the indexed build on small inputs).  value < 0 restores the default.            */
typedef enum VdOption {
    VD_OPT_CULL_SPLIT_MIN = 1,    /* vd_cull_*: inputs of at least this many instances run the split form
                                     (pass 1 -> scan -> pass 2); default 2 Mi                            */
    VD_OPT_CULL_VARIANT = 2,      /* > 0: vd_cull_* always run the fused form, the compacting one with this
                                     many rounds per tile (1, 2, 4, 8, 16; others 32) - a tile-size A/B;
                                     default 0: form and tile size by input size                          */
    VD_OPT_TLAS_INDEX = 10,       /* 0: never use the indexed TLAS build; default 1                       */
    VD_OPT_TLAS_INDEX_MIN = 11,   /* smallest n the indexed build takes; default 6800                     */
    VD_OPT_TLAS_PHASE2 = 12,      /* clusters left at which the indexed build hands over to plain scans;
                                     default 4096                                                        */
    VD_OPT_TLAS_REFRESH = 13,     /* merges between two re-tightenings of the index corners; default 512  */
    VD_OPT_TLAS_GROUPS = 14,      /* workgroups of the plain chain (1 = single workgroup); default by n   */
    VD_OPT_TLAS_SPIN_LIMIT = 15,  /* polls before the several-workgroup chain gives up and the build is
                                     redone on one workgroup (0 forces the redo: tests)                   */
    VD_OPT_TLAS_PROFILE = 17,     /* 1: the indexed build prints its in-kernel cycle counters             */
    VD_OPT_TLAS_CHAIN_LDS = 18,   /* 0: the single-workgroup chain reads its slot arrays from memory even when
                                     they would fit LDS (<= 5600 instances); default 1 (A/B)               */
    VD_OPT_BLAS_LBVH_MAX_DEPTH = 19,/* D >= 1: vd_bvh_build_lbvh* build the DEPTH-BOUNDED topology defined at "LBVH bottom level" below -
                                     max_depth <= D for every input, so D = 23 makes every tree fit the 24-entry stack of the WGSL
                                     traverse_bvh.  Values above 62 are read as 62 (which no input reaches: the unbounded tree's bytes).
                                     Two more launches and 8 more bytes of work memory per triangle; a build is refused
                                     (VD_ERR_INVALID_ARG) when n_tri > 2^(D+1) can not be held.  vd_bvh_lbvh_plan_dev latches the
                                     value.  Default 0: unbounded - the launches, memory and bytes of a library without the option */
    VD_OPT_BLAS_WIDE_PAYLOAD = 30,/* 1: vd_bvh_build moves the 8-byte payload (what meshes above 2^25 triangles use) at
                                     any size (tests); default 0                                                  */
    VD_OPT_BLAS_REFIT_FENCES = 31,/* 1: vd_bvh_refit_planned_dev adds an agent-scope release / acquire fence pair around every arrival-counter
                                     add of its climb, on top of the write-through stores and L1-bypassing loads that carry the boxes
                                     (same bytes; A/B: profiles/blas_refit.md); default 0                                     */
    VD_OPT_TRACE_RAY_RANGE = 20,  /* 1: vd_trace* read VdRay::_pad0 / _pad1 as (t_min, t_max): "Ray intervals" below; default 0   */
    /* 21-23: unassigned (ray binning, chunked ray supply: removed); accepted like every id, change nothing  */
    VD_OPT_TRACE_YIELD = 24,      /* lanes of a wave that wait (at a BLAS leaf, or with a finished ray) before the wave
                                     leaves its stepping loop to serve them; default 16                          */
    VD_OPT_TRACE_WAVES = 25,      /* persistent waves per CU (1..24); default 24                                  */
    VD_OPT_TRACE_AUTO_PREPARE = 27,/* 1 (default): a vd_trace_dev / vd_trace_any_dev call de-indexes the leaf triangles
                                     itself (what vd_trace_prepare_dev does once per scene) when that is cheap next to
                                     the walk: n_rays * 8 >= triangles <= 2 Mi, at most 65 535 meshes.  The 36 B per
                                     triangle live in the context's grow-only scratch (<= 72 MB, kept until
                                     vd_ctx_destroy); 2: up to 16 Mi triangles (576 MB); 0: never                */
    VD_OPT_TRACE_FAN = 29,        /* launches one vd_trace* call runs as (1..4; default 3, and 1 for 15 calls after a call whose rays were all too short to fan out).  Once the rays are handed out, a wave that
                                     is down to a few live rays turns each into jobs - one per TLAS subtree on its stack - for
                                     the next launch's waves: the rays that take thousands of steps stop being what the call
                                     waits for.  Same bytes out (the minimum over (t, visit order) is kept through order keys;
                                     DESIGN.md 3.5).  1 = one launch (A/B).  Calls with at least one ray per lane of the grid
                                     and scenes of >= 64 instances only; 8 B per ray + up to 96 MB of job slots in the context's
                                     grow-only scratch                                                             */
    VD_OPT_TRACE_FAN_SLOTS = 26,  /* upper limit of the fan-out's job slots (default: 2 per ray, at most 2 Mi).  A wave that finds the
                                     list full keeps its rays and runs them to the end; the tests use a small value to get there */
    VD_OPT_TRACE_TIGHT_TLAS = 28, /* 1: vd_trace_prepare_dev builds a PRIVATE top level for the prepared scene over tight
                                     world boxes (the 8 transformed corners of each instance's BLAS root box, WITHOUT the
                                     object-space seed of tlas.rs:39 that makes the reference's leaves overlap at the
                                     origin; padded by 2e-5 of the largest coordinate) and starts rays at its true root.
                                     Every BLAS and the walk inside an instance are unchanged, so hit flags are the
                                     reference's and distances are within north_star's 1e-5 (bit-equal in practice; which
                                     of two triangles at the SAME distance is reported may differ).  NOT the reference's
                                     visit order: default 0, and off in every bit-exact parity run.  Needs
                                     inv_transform = transform^-1 and finite boxes for EVERY instance (checked; one
                                     that fails and the scene keeps its own top level - VdTraceAccelInfo says so) and
                                     2 .. 32 768 instances (else ignored).  1: the top level is clustered by the
                                     agglomerative builder of tlas.rs:56-105 (best tree; the sequential chain: 35 ms for
                                     2 000 instances); 2: an LBVH built on all CUs (~0.1 ms, <= 32 767 instances) - the form
                                     for scenes that move.  The private top level is a snapshot of the instances:
                                     vd_trace_accel_update_dev rebuilds it after they moved, vd_trace_accel_refit_dev
                                     refits it.  vd_trace_prepare_wide_dev: 1 and 2 both select the LBVH, over
                                     VdTlasNodeWide, for 2 .. VD_TLAS_WIDE_MAX_INSTANCES instances.                */
    VD_OPT_COUNT_ = 32
} VdOption;
int         vd_ctx_set_option(VdCtx* ctx, int option /* VdOption */, int64_t value);

/* HIP -> wgpu hand-off.  The renderer owns `draw_cmd_buffer`
 * (ResizableBuffer<DrawIndexedIndirect>, crates/components/src/buffer.rs:42-47, created in
 * app.rs:167-171); to let Geometry::record consume the commands without a PCIe round trip the
 * Vulkan allocation behind it is exported as an opaque fd (VK_KHR_external_memory_fd) and mapped
 * here; the returned device pointer is then passed as `d_out` of vd_cull_emit_dev /
 * vd_cull_compact_dev.  The fd is consumed on success (Vulkan/HIP convention).  Ordering
 * against the consumer: the external semaphores below (no CPU wait), or vd_ctx_synchronize.  */
typedef struct VdExternalBuffer VdExternalBuffer;
int vd_import_external_buffer(VdCtx* ctx, int opaque_fd, uint64_t size_bytes, VdExternalBuffer** out_handle,
                              void** out_device_ptr);
int vd_release_external_buffer(VdCtx* ctx, VdExternalBuffer* handle);

/* ... and its ordering.  The renderer's frame is ONE queue.submit followed by present
 * (crates/app/src/app.rs:334-348); a CPU wait on each side of a 0.27 ms cull would be most of the frame.  A Vulkan
 * semaphore exported as an opaque fd (VK_KHR_external_semaphore_fd; binary, or timeline with is_timeline != 0) is
 * imported once, and then
 *     vd_wait_external_semaphore_async(ctx, frame_ready, f)      the submit that wrote instances / camera has finished
 *     vd_cull_compact_dev(ctx, ..., d_out = imported buffer, ...)
 *     vd_signal_external_semaphore_async(ctx, draws_ready, f)    Geometry::record's submit waits for this one
 * are three operations ENQUEUED on the context's stream: no host round trip.  `value` is the timeline point (ignored
 * for a binary semaphore).  The fd is consumed on success.  vd_release_external_semaphore synchronises the stream
 * first (queued waits / signals refer to the semaphore).
 * What this image can test: argument validation and the error path of a descriptor that is not a semaphore
 * (tests/test_gpu_tlas_trace.py), and - round 6 - an import of a REAL kernel sync object (what a Vulkan binary semaphore
 * exported as an opaque fd is on amdgpu; tests/cpp/external_semaphore_test.cpp makes one with DRM_IOCTL_SYNCOBJ_CREATE):
 * the HIP runtime of this image answers hipImportExternalSemaphore with "operation not supported" (binary) and
 * "invalid argument" (timeline), so VD_ERR_HIP is what these calls return on this platform today and no functional
 * round trip is claimed (profiles/r06_external_semaphore_probe.log; the test runs the signal and the wait round trip
 * on a runtime that accepts the import).  The calls are hipImportExternalSemaphore /
 * hip{Wait,Signal}ExternalSemaphoresAsync / hipDestroyExternalSemaphore and nothing else.  Until a runtime implements
 * them, order the frame through the host without blocking the render thread: INTEGRATION.md 5.                       */
typedef struct VdExternalSemaphore VdExternalSemaphore;
int vd_import_external_semaphore(VdCtx* ctx, int opaque_fd, int is_timeline, VdExternalSemaphore** out_handle);
int vd_wait_external_semaphore_async(VdCtx* ctx, VdExternalSemaphore* handle, uint64_t value);
int vd_signal_external_semaphore_async(VdCtx* ctx, VdExternalSemaphore* handle, uint64_t value);
int vd_release_external_semaphore(VdCtx* ctx, VdExternalSemaphore* handle);

/* Ordering that WORKS on this platform (NEW, round 6): a word of shared memory and the host.
 * The external-semaphore import above is refused by this image's HIP runtime (profiles/r06_external_semaphore_probe.log),
 * so the frame's two hand-overs have a second form:
 *   renderer -> HIP, GPU side only: the renderer's upload submit ends by writing the frame number f into a 32-bit word of a
 *     buffer both APIs see (vkCmdFillBuffer into an allocation imported with vd_import_external_buffer - the draw buffer's
 *     own tail will do); vd_wait_value32_async(ctx, d_word, f) holds the context's stream until *d_word >= f (unsigned,
 *     hipStreamWaitValue32 / GTE), then the cull runs.  No host thread waits, none is woken.
 *   HIP -> renderer: Vulkan cannot wait on a memory word; vd_host_callback_async(ctx, callback, user) runs callback(user) on a thread
 *     of the HIP runtime once the stream reaches it (hipLaunchHostFunc) - it calls vkSignalSemaphore on a timeline semaphore
 *     the frame's queue.submit waits for.  The callback must not call into HIP or this library.
 *   vd_write_value32_async(ctx, d_word, v) is the stream-side store (hipStreamWriteValue32): a second HIP context, or a
 *     test, stands in for the renderer's queue with it.
 * Enqueue-only, like the per-frame entry points; d_word must be 4-byte aligned device-accessible memory of the context's
 * device (ordinary allocations and imported external buffers both work here: tests/cpp/frame_ordering_test.cpp).  Stream
 * memory operations are not captured into HIP graphs: keep them outside a captured frame.  A wait nobody ever satisfies
 * holds the stream for good (vd_ctx_synchronize and everything that synchronises would not return): the protocol on the
 * word - monotone frame numbers, written once per frame by the other queue - is the caller's.                          */
typedef void (*VdHostFn)(void* user);
int vd_wait_value32_async(VdCtx* ctx, const uint32_t* d_word, uint32_t value);
int vd_write_value32_async(VdCtx* ctx, uint32_t* d_word, uint32_t value);
int vd_host_callback_async(VdCtx* ctx, VdHostFn callback, void* user);

/* ------------------------------------------------------------------------------------ */
/* Cull + emit                                                      */
/* ------------------------------------------------------------------------------------ */
/* C1/C2 — replaces the `emit_draws` compute dispatch recorded by EmitDraws::record
 * (crates/app/src/pass/visibility.rs:233-254; shaders/emit_draws.wgsl:13-64).
 * Writes out[0..n_inst): every slot, culled ones with instance_count = 0.
 * mesh ids >= n_mesh are clamped to n_mesh-1 (the reference leaves this to Vulkan robust
 * buffer access, i.e. undefined).                                                       */
int vd_cull_emit(VdCtx* ctx, const VdCameraUniform* camera,
                 const VdMeshInfo* meshes, uint32_t n_mesh,
                 const VdInstance* instances, uint32_t n_inst,
                 VdDrawIndexedIndirect* out);
int vd_cull_emit_dev(VdCtx* ctx, const VdCameraUniform* camera /* host */,
                     const VdMeshInfo* d_meshes, uint32_t n_mesh,
                     const VdInstance* d_instances, uint32_t n_inst,
                     VdDrawIndexedIndirect* d_out);

/* C1+C3 fused — cull and emit only the survivors, in ascending instance order:
 *   S = [i : emit_draws(i).instance_count == 1];  out[k] = emit_draws(S[k]);  *count = |S|.
 * base_instance keeps the original instance index, so shaders/visibility.wgsl:33 is
 * unchanged.  If pad_tail != 0, out[count..n_inst) is filled with zeroed commands
 * (instance_count = 0) so that the unchanged
 * `multi_draw_indexed_indirect(buf, 0, N)` consumer (visibility.rs:188-192) stays valid;
 * with pad_tail == 0 only out[0..count) is written (for multi_draw_indexed_indirect_count).
 * `out` must hold n_inst commands either way.
 * When a launch fails: the ordered scans behind the compaction wait for each other across workgroups, and every
 * such wait is bounded by the wall clock (two seconds).  If one times out (a workgroup of the launch was lost or
 * stalled) no list is written, *count becomes 0 - with pad_tail the whole buffer is zeroed, so neither consumer
 * draws anything, least of all a mix of this frame's and the last frame's commands - and the context remembers:
 * vd_cull_compact returns VD_ERR_HIP for that very call; after a *_dev call the NEXT vd_cull_compact* /
 * vd_compact_draws* call on the context returns VD_ERR_HIP once (and resets the scan state) instead of launching.
 * One case cannot be turned into a count of 0: a launch that loses the workgroup that writes the count leaves the
 * value its first workgroup pre-stored, 0xffffffff - larger than any n_inst.  vd_cull_compact returns VD_ERR_HIP
 * for it as well; pad_tail zeroes the whole buffer for it; a caller that hands the count straight to
 * multi_draw_indexed_indirect_count should clamp it to 0 when it exceeds n_inst.                              */
int vd_cull_compact(VdCtx* ctx, const VdCameraUniform* camera,
                    const VdMeshInfo* meshes, uint32_t n_mesh,
                    const VdInstance* instances, uint32_t n_inst,
                    VdDrawIndexedIndirect* out, uint32_t* out_count, int pad_tail);
int vd_cull_compact_dev(VdCtx* ctx, const VdCameraUniform* camera /* host */,
                        const VdMeshInfo* d_meshes, uint32_t n_mesh,
                        const VdInstance* d_instances, uint32_t n_inst,
                        VdDrawIndexedIndirect* d_out, uint32_t* d_out_count, int pad_tail);

/* Shard variants (NEW): the instance array is a contiguous shard
 * [first_instance, first_instance + n_inst) of a larger scene; base_instance is written as the
 * GLOBAL index so that shards concatenated in rank order equal the single-GPU result.      */
int vd_cull_emit_shard_dev(VdCtx* ctx, const VdCameraUniform* camera /* host */,
                           const VdMeshInfo* d_meshes, uint32_t n_mesh,
                           const VdInstance* d_instances, uint32_t n_inst, uint32_t first_instance,
                           VdDrawIndexedIndirect* d_out);
int vd_cull_compact_shard_dev(VdCtx* ctx, const VdCameraUniform* camera /* host */,
                              const VdMeshInfo* d_meshes, uint32_t n_mesh,
                              const VdInstance* d_instances, uint32_t n_inst, uint32_t first_instance,
                              VdDrawIndexedIndirect* d_out, uint32_t* d_out_count, int pad_tail);

/* Several views of one scene (NEW; no reference counterpart - the reference renders one view): the main camera plus
 * shadow cascades or cube-map faces, a stereo pair, the jittered and the unjittered camera of a TAA pair.  The
 * instances are read ONCE for all n_views cameras (2..VD_MAX_VIEWS; 1 forwards to vd_cull_compact_dev), then the
 * ordered list of every view is written as vd_cull_compact_dev writes it.  Pinned exactly, because views are independent:
 *   view v's list   = d_out[v * out_stride .. + d_out_counts[v]),  ascending instance order, base_instance = index
 *                   == the bytes vd_cull_compact_dev(cameras[v], ..., d_out + v * out_stride, d_out_counts + v, pad_tail) writes;
 *   pad_tail != 0   zeroes [count, n_inst) of every view.  Nothing else in d_out is written: not the slots
 *                   [n_inst, out_stride) of a view and, without pad_tail, not the slots behind its count.
 * out_stride (in commands, >= n_inst) separates two views' lists: n_inst packs them, a larger value gives every view its
 * own buffer region (an EmitDrawsResource per view).  Always the two-pass form, at every size: one multi-view
 * cull-to-bitmask pass, then one expansion per view - n_views + 1 launches (2 n_views + 1 with pad_tail), no scan, no wait
 * between workgroups, hence no "gave up" state.  Like the other per-frame entry points it only enqueues kernels on the
 * context's stream once its scratch exists (first call, or a larger scene), so it can be captured into a HIP graph; the
 * cameras are baked in by value.  vd_last_gpu_ms_stage: 0 = the shared pass, 1 = all expansions.
 * VD_ERR_INVALID_ARG: null ctx / cameras / meshes / counts, n_views == 0 or > VD_MAX_VIEWS, n_mesh == 0,
 * out_stride < n_inst, null instances / out with n_inst > 0.  n_inst == 0 sets all n_views counts to 0.
 * What the shared pass costs per view, and where it stops being free (K = 4): DESIGN.md §3.1, profiles/cull_views.md. */
#define VD_MAX_VIEWS 8
int vd_cull_compact_views_dev(VdCtx* ctx, const VdCameraUniform* cameras /* host, n_views */, uint32_t n_views,
                              const VdMeshInfo* d_meshes, uint32_t n_mesh,
                              const VdInstance* d_instances, uint32_t n_inst,
                              VdDrawIndexedIndirect* d_out, uint64_t out_stride /* commands between two views' lists, >= n_inst */,
                              uint32_t* d_out_counts /* device, n_views words */, int pad_tail);
/* host-pointer form, staged through the context and synchronous, like vd_cull_compact */
int vd_cull_compact_views(VdCtx* ctx, const VdCameraUniform* cameras, uint32_t n_views,
                          const VdMeshInfo* meshes, uint32_t n_mesh,
                          const VdInstance* instances, uint32_t n_inst,
                          VdDrawIndexedIndirect* out, uint64_t out_stride, uint32_t* out_counts, int pad_tail);

/* Multi-GPU wire format (NEW): the exchange between GPUs carries ONE BIT per
 * instance instead of a 20-byte command.
 *   vd_cull_mask_dev    runs the cull and writes bit i%64 of d_mask[i/64] = emit_draws(i).instance_count
 *                       (ceil(n_inst/64) words; padding bits are 0).
 *   vd_expand_mask_dev  rebuilds the ordered compacted draw list of a whole scene from the
 *                       concatenated shard masks: shard r covers instances [r*shard_size,
 *                       min(n_total, (r+1)*shard_size)) and owns ceil(shard_size/64) words; the
 *                       per-instance mesh ids (d_mesh_ids[n_total], id_bytes = 1, 2 or 4 bytes each;
 *                       static per scene, replicated once) supply the command fields.  Output ==
 *                       vd_cull_compact on the whole scene, bit for bit.                          */
int vd_cull_mask_dev(VdCtx* ctx, const VdCameraUniform* camera /* host */,
                     const VdMeshInfo* d_meshes, uint32_t n_mesh,
                     const VdInstance* d_instances, uint32_t n_inst, uint64_t* d_mask);
int vd_expand_mask_dev(VdCtx* ctx, const uint64_t* d_mask, uint32_t n_total, uint32_t shard_size,
                       const void* d_mesh_ids, uint32_t id_bytes, const VdMeshInfo* d_meshes,
                       uint32_t n_mesh, VdDrawIndexedIndirect* d_out, uint32_t* d_out_count);

/* Indices-only wire format (NEW; SURVEY.md §8e "gather only survivor indices (4 B each) and rebuild
 * commands locally from replicated mesh_ids"): pays off against the bitmask when fewer than 1 instance
 * in 32 survives.
 *   vd_mask_to_indices_dev  ascending list of the set bits of a shard mask (ceil(n_inst/64) words) as
 *                           GLOBAL instance indices first_instance + i; *d_out_count = their number.
 *                           Words [*d_out_count, n_inst) of d_out_indices are NOT written.
 *   vd_indices_to_draws_dev d_out[k] = the command emit_draws writes for instance d_indices[k] with
 *                           instance_count = 1 (mesh fields through d_mesh_ids, as vd_expand_mask_dev).
 * vd_indices_to_draws(concat over shards of vd_mask_to_indices(vd_cull_mask(shard))) == vd_cull_compact
 * on the whole scene, bit for bit.                                                                  */
int vd_mask_to_indices_dev(VdCtx* ctx, const uint64_t* d_mask, uint32_t n_inst, uint32_t first_instance,
                           uint32_t* d_out_indices, uint32_t* d_out_count);
int vd_indices_to_draws_dev(VdCtx* ctx, const uint32_t* d_indices, uint32_t n_indices, const void* d_mesh_ids,
                            uint32_t id_bytes, uint32_t n_total, const VdMeshInfo* d_meshes, uint32_t n_mesh,
                            VdDrawIndexedIndirect* d_out);

/* C3 alone — ordered compaction of an existing emit_draws output (same definition).     */
int vd_compact_draws_dev(VdCtx* ctx, const VdDrawIndexedIndirect* d_in, uint32_t n,
                         VdDrawIndexedIndirect* d_out, uint32_t* d_out_count);

/* Instanced draw lists (NEW; no reference counterpart - the reference submits one single-instance command per instance):
 * ONE command per MESH with instance_count = the visible instances of that mesh, and a 4-byte instance id per survivor,
 * grouped by mesh, that the vertex shader indexes with instance_index (shaders/visibility.wgsl:33 becomes
 * `instances[visible_ids[in.instance_index]]`: INTEGRATION.md).  n_mesh commands + 4 B per survivor instead of 20 B per
 * survivor, and n_mesh draws for the consumer instead of one per survivor.  A pure function of the existing list:
 *   S      = the ascending list of instances i with emit_draws(i).instance_count == 1
 *            (vd_batch_mask_dev: the set bits of d_mask, bit i % 64 of word i / 64 = instance i);
 *   mid(i) = min(mesh id of i, n_mesh - 1) - the clamp emit_draws, the oracle and the id table already apply;
 *   S_m    = the sub-list of S with mid == m, still ascending.
 *   d_out_instance_ids[0 .. |S|)  = S_0 || S_1 || ... || S_{n_mesh-1}: a STABLE sort of S by mesh.  Words [|S|, n_inst)
 *                                   are NOT written.
 *   d_out_cmds[m]                 = { meshes[m].index_count, |S_m|, meshes[m].base_index, meshes[m].vertex_offset,
 *                                   sum of |S_k| over k < m } for EVERY m < n_mesh: empty meshes are included with
 *                                   instance_count = 0, so multi_draw_indexed_indirect(buf, 0, n_mesh) is valid as it
 *                                   stands.  Exactly n_mesh commands are written.
 *   *d_out_count                  = |S|.
 * n_inst == 0: the n_mesh commands are written with instance_count = 0 and base_instance = 0, the count is 0.
 * VD_ERR_INVALID_ARG: null ctx / camera / meshes / cmds / count; n_mesh == 0 or n_mesh > VD_BATCH_MAX_MESHES (the limit
 * of the one-digit counting sort: a wave-private table of n_mesh counters lives in LDS; a second digit is future work);
 * id_bytes not 1, 2 or 4; null instances / mask / ids / instance-ids with n_inst > 0.  A refused call writes nothing.
 * The padding bits of the last mask word are zero on input, as vd_cull_mask_dev writes them.
 *   vd_batch_mask_dev  groups ANY visibility mask (vd_cull_mask_dev, vd_occlusion_mask_dev, ...) with a caller-supplied
 *                      mesh-id table (n_inst ids of id_bytes = 1, 2 or 4 bytes; clamped to n_mesh - 1 as above).
 *   vd_cull_batch_dev  cull + group in ONE read of the instances: pass 1 of the two-launch step (cull to bitmask, mesh-id
 *                      table, unchanged), then the grouping below.  Always this split form, at every size.
 *   vd_cull_batch      host pointers, staged through the context and synchronous, like vd_cull_compact; out_instance_ids
 *                      holds n_inst words of which [0, *out_count) are written.
 * The grouping is a stable counting sort in four launches: every wave owns one contiguous range of instances and counts
 * its survivors per mesh in LDS (one row of a [wave][mesh] table); a scan down the rows of every column; a scan over the
 * mesh totals by ONE workgroup, which also writes the n_mesh commands and the count; every wave walks its range again and
 * stores each id at cursor[mesh] + its rank among the same-mesh survivors of its 64-instance round (ballots, no atomics).
 * No wait of one workgroup on another, hence no "gave up" state and no use of the scan-fault word; no global atomic, so
 * the bytes are identical from run to run.  Once its scratch exists (first call, or more meshes) a call only enqueues
 * kernels on the context's stream, so it can be captured into a HIP graph; the camera is baked in by value.
 * vd_last_gpu_ms_stage (vd_cull_batch_dev): 0 = pass 1, 1 = everything after it.
 * OUT OF SCOPE: more than VD_BATCH_MAX_MESHES meshes (needs a second sort digit); a multi-view form and a shard /
 * vd_dist_* form; dropping empty meshes from the command array; pad_tail (nothing behind |S| is ever written).
 * Measured times against vd_cull_compact_dev: DESIGN.md §3.1, profiles/cull_batch.md.                                  */
#define VD_BATCH_MAX_MESHES 4096u
int vd_batch_mask_dev(VdCtx* ctx, const uint64_t* d_mask, uint32_t n_inst,
                      const void* d_mesh_ids, uint32_t id_bytes /* 1, 2, 4 */,
                      const VdMeshInfo* d_meshes, uint32_t n_mesh,
                      VdDrawIndexedIndirect* d_out_cmds /* n_mesh */,
                      uint32_t* d_out_instance_ids /* n_inst */,
                      uint32_t* d_out_count);
int vd_cull_batch_dev(VdCtx* ctx, const VdCameraUniform* camera /* host */,
                      const VdMeshInfo* d_meshes, uint32_t n_mesh,
                      const VdInstance* d_instances, uint32_t n_inst,
                      VdDrawIndexedIndirect* d_out_cmds, uint32_t* d_out_instance_ids, uint32_t* d_out_count);
int vd_cull_batch(VdCtx* ctx, const VdCameraUniform* camera,
                  const VdMeshInfo* meshes, uint32_t n_mesh,
                  const VdInstance* instances, uint32_t n_inst,
                  VdDrawIndexedIndirect* out_cmds, uint32_t* out_instance_ids, uint32_t* out_count);

/* ------------------------------------------------------------------------------------ */
/* BLAS build                                                       */
/* ------------------------------------------------------------------------------------ */
/* Replaces `BvhBuilder::new(vertices, indices).build()` (crates/bvh/src/blas.rs:51-103),
 * called from MeshPool::add (crates/pools/src/mesh/mod.rs:320-321).
 *   verts_xyz      n_vert * 3 floats
 *   indices_inout  n_tri * 3 u32; permuted in place exactly as blas.rs:95-100 does
 *   out_nodes      capacity node_cap (>= 2*n_tri as the reference allocates, blas.rs:52)
 *   out_n_nodes    number of nodes used (`nodes.truncate(pool)`, blas.rs:93); node 1 is
 *                  the reference's never-used all-zero slot
 * No byte of out_nodes past n_nodes is written.
 * VD_ERR_DEGENERATE where the reference would crash.
 *
 * vd_bvh_build_dev takes device pointers but - unlike the per-frame `*_dev` entry points - it
 * BLOCKS: it returns when the build is complete on the ctx stream, out_n_nodes is a HOST pointer,
 * and errors (degenerate input, bad index) are reported by its return value.  The builder is a
 * load-time call in the reference (MeshPool::add, mesh/mod.rs:320-345, before the first frame), the
 * level loop reads one 32-byte control word per level back to size the next level's launches, and
 * the DFS pre-order numbering of the top tree (blas.rs:110-112) is a host pass that overlaps the
 * device's phase B; it cannot be captured into a HIP graph.  Builds of different meshes overlap by
 * using one VdCtx (= one stream) per concurrent build.                                       */
int vd_bvh_build(VdCtx* ctx, const float* verts_xyz, uint32_t n_vert,
                 uint32_t* indices_inout, uint32_t n_tri,
                 VdBvhNode* out_nodes, uint32_t node_cap, uint32_t* out_n_nodes);
int vd_bvh_build_dev(VdCtx* ctx, const float* d_verts_xyz, uint32_t n_vert,
                     uint32_t* d_indices_inout, uint32_t n_tri,
                     VdBvhNode* d_out_nodes, uint32_t node_cap, uint32_t* out_n_nodes /* host */);

/* LBVH bottom level (NEW, NOT the reference's tree): a BLAS for a mesh whose TRIANGLES change every frame - fracture,
 * procedural geometry, marching cubes, a streamed LOD, a cloth that tears - where vd_bvh_build's chain of dependent
 * launches and host round trips is too dear and the refit below does not apply.  The array has the reference's BvhNode
 * layout and node numbering, so every consumer of a BLAS takes it as it is: the WGSL traverse_bvh, vd_trace*,
 * vd_trace_prepare*, vd_traverse_iter_dev, vd_bvh_refit_plan_dev.  The tree is a function of the input alone:
 *   box       of a triangle: its three corners folded from (+1e30, -1e30) with the NaN-ignoring min / max of
 *             calculate_bounds and the refit (tie rule -0 < +0).  A corner whose index is >= n_vert counts as a NaN
 *             vertex: it is ignored, never read, and counted in n_bad_indices.
 *   code      the key of vd_tlas_build_lbvh* applied to the triangle boxes: centre 0.5 * (min + max) in float32, 10 bits
 *             per axis of the extent of the finite centres, x in the highest bit of each triple; a centre with a
 *             non-finite coordinate gets 0x3fffffff.
 *   order     stable sort by code (equal codes keep input order); indices_inout is rewritten in that order, whole triples.
 *   topology  the binary radix tree (Karras 2012) over the 64-bit keys code << 32 | sorted position.  A radix-tree node
 *             that covers <= 3 sorted positions is a LEAF with left_first = its first position and count = 1..3 (the
 *             reference's `count <= 3`, blas.rs:106); its radix descendants are not emitted.
 *   numbering the reference's (blas.rs:105-128): node 0 is the root, slot 1 the never-used all-zero node; an interior
 *             node has count = 0 and its children at left_first and left_first + 1, a pair allocated when the node is
 *             subdivided, before anything below it; then the whole left subtree, then the right.  So every child id is
 *             greater than its parent's, n_nodes = 2 + 2 * (interior nodes) <= max(2, 2 * n_tri), and n_tri <= 3 gives
 *             n_nodes = 2 with node 0 a leaf.
 *   boxes     a leaf's is the union of its triangles' boxes, an interior node's the union of its children's:
 *             vd_bvh_refit(lbvh(x), x) changes no byte.
 *   depth-bounded topology   with VD_OPT_BLAS_LBVH_MAX_DEPTH = D >= 1 (default 0: the topology above), box, code, order, numbering
 *             and boxes stay as defined; only the topology changes.  Let needr(k) = 0 for k <= 3, else bits(k - 1) - 1: the depth
 *             of the radix tree over the integers 0 .. k - 1 cut off at nodes of <= 3 positions.  Top-down, a node covers the
 *             sorted positions [lo, hi] at depth d, k = hi - lo + 1 of them.  k <= 3: a leaf, as above.  In RADIX MODE (the
 *             root's) let s be the split above: the first position whose key code << 32 | position has the highest bit in which
 *             the end keys differ.  If d + 1 + needr(max(s - lo, hi - s + 1)) <= D the node splits at s and both children are in
 *             radix mode; otherwise it is a SWITCH NODE: it and everything below it are in POSITION MODE with base = its lo.  In
 *             position mode the split is the radix split over p - base: b = the highest bit in which lo - base and hi - base
 *             differ, s = base + (((lo - base) >> b | 1) << b).  d + needr(k) <= D holds for every node - at the root that is
 *             needr(n_tri) <= D, i.e. n_tri <= 2^(D+1); a radix child keeps it by the rule; a position subtree is exactly
 *             needr(k) deep - so max_depth <= D FOR EVERY INPUT.  A build with needr(n_tri) > D is refused before anything is
 *             launched (VD_ERR_INVALID_ARG; the message names the smallest bound that works): D = 23 takes every n_tri <=
 *             VD_BVH_LBVH_MAX_TRIANGLES.  For D >= 53 the rule cannot fire (30 code bits, then at most 2^24 positions).  The tree
 *             is still a function of the input alone, the call still only enqueues: two more launches, 8 more bytes of work memory
 *             per triangle (the same warm-up rule for graph capture).  On real meshes D = 23 moves a few dozen positions (the
 *             helmet: 5 switch nodes over 34 of 15 452 positions; trace rate within 1 % of the unbounded tree's): profiles/blas_lbvh_bounded.md.
 * No byte of out_nodes past n_nodes is written.  The build is TOTAL: there is no VD_ERR_DEGENERATE - duplicate triangles,
 * collinear centres, NaN and infinite vertices all give a valid tree.
 *
 * vd_bvh_build_lbvh_dev ONLY ENQUEUES on the context's stream: no host read-back, and no allocation once the context's
 * grow-only work memory has reached the size of the largest n_tri (one warm-up call at that size), so it can be captured
 * into a HIP graph and replayed.  d_result is DEVICE memory, written by the build.  VD_ERR_INVALID_ARG before anything is
 * launched for: a null pointer, n_tri == 0, n_tri > VD_BVH_LBVH_MAX_TRIANGLES, node_cap < max(2, 2 * n_tri), a d_out_nodes
 * that is not 16-byte aligned.
 *   max_depth  edges on the longest path from node 0 to a leaf.  The WGSL traverse_bvh (bvh.wgsl:35-75) pushes the root, and
 *              for every interior node it enters BOTH children before it pops one, so a ray that enters both children all
 *              the way down the deepest path holds max_depth + 1 entries.  Its stack (stack.wgsl, STACK_LEN = 24) is
 *              UNCHECKED: use the tree there only when max_depth <= 23.  The UNBOUNDED LBVH over a real mesh does NOT pass
 *              that: 24 for the 15 k-triangle helmet, 24 to 34 for the knots of profiles/blas_lbvh.md.  A renderer whose
 *              shader walks the array sets VD_OPT_BLAS_LBVH_MAX_DEPTH to 23 once, and every build then passes by
 *              construction.  vd_trace*'s 128 entries (with its overflow pass behind them) hold any tree this build can
 *              make: 62 key bits bound max_depth by 62.
 * vd_bvh_build_lbvh: host pointers, synchronous: stage, build, copy back.  VD_ERR_INVALID_ARG when n_bad_indices != 0.
 * Which builder for which mesh, and the trace rate through either tree: profiles/blas_lbvh.md.                        */
#define VD_BVH_LBVH_MAX_TRIANGLES (1u << 24)
typedef struct VdBvhLbvhResult { uint32_t n_nodes, n_bad_indices, max_depth, _pad; } VdBvhLbvhResult;
int vd_bvh_build_lbvh_dev(VdCtx* ctx, const float* d_verts_xyz, uint32_t n_vert, uint32_t* d_indices_inout, uint32_t n_tri,
                          VdBvhNode* d_out_nodes, uint32_t node_cap, VdBvhLbvhResult* d_result /* DEVICE */);
int vd_bvh_build_lbvh(VdCtx* ctx, const float* verts_xyz, uint32_t n_vert, uint32_t* indices_inout, uint32_t n_tri,
                      VdBvhNode* out_nodes, uint32_t node_cap, uint32_t* out_n_nodes);

/* Batched LBVH bottom level: MANY meshes rebuilt in one call, every mesh's triangle count read from DEVICE memory - the shards
 * of a fracture, the chunks of a marching-cubes volume, streamed LODs - where a vd_bvh_build_lbvh_dev per mesh pays its chain
 * of launches per mesh and needs the count on the host.  Plan once per layout (pointers and capacities), then one call per
 * frame (the idiom of vd_bvh_refit_plan_dev below).
 * DEFINITION.  For item m let T_m = min(d_n_tri[m], tri_cap_m): a count ABOVE THE CAPACITY IS READ AS THE CAPACITY; d_n_tri ==
 * NULL means every tri_cap.  Then nodes[0 .. n_nodes), the first 3 * T_m indices and d_results[m] (all 16 bytes, _pad 0) are
 * byte for byte what vd_bvh_build_lbvh_dev(verts_xyz, n_vert, indices_inout, T_m, nodes, node_cap, &d_results[m]) writes for
 * that mesh alone - box, code (the extent is each mesh's own), order, topology, numbering and boxes as defined above, node
 * ids and leaf positions mesh-local.  No byte of nodes past n_nodes and no index past 3 * T_m is written.
 *   T_m == 0    is legal here (a shard can vanish): d_results[m] is all zero (n_nodes == 0) and no node is written; a consumer
 *               skips such a mesh - it has no node 0.
 *   mesh_info   optional.  Its min / max become what MeshPool::calculate_bounds gives over ALL n_vert vertices from
 *               (+inf, -inf), NaN ignored - the definition and the device code of vd_bvh_refit_planned_dev - whatever T_m is; no
 *               other field is touched.
 * vd_bvh_lbvh_plan_dev           once per layout.  BLOCKS: validates, uploads the descriptor table and allocates ALL work memory
 *                                inside the plan, sized by the capacities (each mesh's slots are rounded up to 256; about 110 B
 *                                per slot).  The plan keeps the items' POINTERS, not their data.  VD_ERR_INVALID_ARG with
 *                                items[m].status set (no plan is returned) for: a null verts_xyz / indices_inout / nodes;
 *                                tri_cap == 0; node_cap < max(2, 2 * tri_cap); nodes not 16-byte aligned; the capacities, each
 *                                rounded up to 256, adding up to more than VD_BVH_LBVH_MAX_TRIANGLES (the item that crosses
 *                                it); under VD_OPT_BLAS_LBVH_MAX_DEPTH = D, needr(tri_cap) > D (T_m <= tri_cap then keeps every
 *                                count on the device inside the bound); and, without a status, n_items >
 *                                VD_BVH_LBVH_BATCH_MAX_ITEMS.  The option is LATCHED here: it sizes the plan's memory and fixes
 *                                its launch list, and changing it later does not touch an existing plan.  The items are judged
 *                                before the context is looked at, so a null ctx with a bad item names that item too.
 *                                n_items == 0 is VD_OK: a plan that does nothing.
 * vd_bvh_build_lbvh_planned_dev  ONLY ENQUEUES on the context's stream: no host read, no allocation, nothing on the host that
 *                                depends on the counts - it can be captured into a HIP graph and replayed after d_n_tri has
 *                                changed.  The number of launches depends on the plan alone (19 or 23 kernels by its capacities, 21 or 25
 *                                for a depth-bounded plan, no memset, one more kernel when an item carries a mesh_info), never on
 *                                n_items or the counts.  A null
 *                                plan or d_results is VD_ERR_INVALID_ARG.  One build of a plan at a time (calls on one stream
 *                                are ordered).
 * vd_bvh_lbvh_plan_release       synchronises the stream first (a queued build uses the plan's memory).
 * vd_bvh_build_lbvh_batch        host pointers inside the items (mesh_info too), host n_tri (may be NULL) and results;
 *                                synchronous: stage, plan, build, copy back, release.  VD_ERR_INVALID_ARG with items[m].status
 *                                set when a mesh has n_bad_indices != 0 (nothing is copied back), as vd_bvh_build_lbvh.
 * Per-frame order: INTEGRATION.md 3d.  Measured against a loop of single builds: profiles/blas_lbvh_batch.md.               */
#define VD_BVH_LBVH_BATCH_MAX_ITEMS (1u << 16)
typedef struct VdBvhLbvhBatchItem {
    const float* verts_xyz;     /* n_vert * 3, read at every build                                   */
    uint32_t*    indices_inout; /* tri_cap * 3, mesh-local; the first 3 * n_tri are permuted in place */
    VdBvhNode*   nodes;         /* node_cap >= max(2, 2 * tri_cap), 16-byte aligned                   */
    VdMeshInfo*  mesh_info;     /* optional: min / max refreshed as vd_bvh_refit_planned_dev does     */
    uint32_t     n_vert, tri_cap, node_cap;
    int32_t      status;        /* written by the plan call                                           */
} VdBvhLbvhBatchItem;
typedef struct VdBvhLbvhPlan VdBvhLbvhPlan;
int vd_bvh_lbvh_plan_dev(VdCtx* ctx, VdBvhLbvhBatchItem* items /* host array, device pointers inside */, uint32_t n_items,
                         VdBvhLbvhPlan** out);
int vd_bvh_build_lbvh_planned_dev(VdCtx* ctx, const VdBvhLbvhPlan* plan, const uint32_t* d_n_tri /* DEVICE, n_items; NULL = every tri_cap */,
                                  VdBvhLbvhResult* d_results /* DEVICE, n_items */);
int vd_bvh_lbvh_plan_release(VdCtx* ctx, VdBvhLbvhPlan* plan);
int vd_bvh_build_lbvh_batch(VdCtx* ctx, VdBvhLbvhBatchItem* items /* host pointers inside */, uint32_t n_items,
                            const uint32_t* n_tri /* host, may be NULL */, VdBvhLbvhResult* results /* host */);

/* Batched BLAS build (NEW): K meshes in ONE build.  MeshPool::add builds one BLAS per mesh at load
 * (crates/pools/src/mesh/mod.rs:309-351: Sponza-class scenes are hundreds of small meshes) and a
 * single build has a fixed cost of launches and host round trips that dwarfs a 15 k-triangle mesh.
 * Here the meshes' triangles lie side by side in one position space and every pass of the builder -
 * the level loop (one host round trip per level for the WHOLE batch), the mid tier, the small
 * subtrees - runs once for all of them; meshes of <= 2048 / <= 512 triangles start in those tiers
 * directly.  Each mesh's nodes and permuted indices are exactly what vd_bvh_build gives for that
 * mesh alone (mesh-local node ids and leaf positions, node 1 all-zero).
 *   items          host array; per mesh: vertices, mesh-local indices (permuted in place), and either
 *                  its own node array (out_nodes, node_cap) or out_nodes = NULL = PACKED: the mesh's
 *                  nodes follow the previous packed mesh's in `packed_nodes`, from `packed_first` on -
 *                  MeshPool's `bvh_index = bvh_nodes.len()` bookkeeping (mesh/mod.rs:320-345);
 *                  written back: out_n_nodes, out_first_node (= MeshInfo.bvh_index when packed), status
 *   packed_nodes   shared node buffer of `packed_cap` nodes (may be NULL when no item is packed)
 *   out_packed_end one past the last packed node written (host pointer, may be NULL)
 * _dev: every pointer inside the items and packed_nodes are device pointers; blocks like
 * vd_bvh_build_dev.  An error fails the whole batch (nothing is to be used); items[m].status names the
 * mesh when the error has one (bad index, capacity, VD_ERR_DEGENERATE: of several degenerate meshes
 * the first in the batch among those found when the build stopped; vd_last_error says "mesh M" too). */
typedef struct VdBvhBatchItem {
    const float* verts_xyz;        /* n_vert * 3 floats                                     */
    uint32_t*    indices_inout;    /* n_tri * 3 u32, mesh-local                             */
    VdBvhNode*   out_nodes;        /* NULL = packed                                         */
    uint32_t     n_vert, n_tri, node_cap;
    uint32_t     out_n_nodes;      /* written                                               */
    uint32_t     out_first_node;   /* written                                               */
    int32_t      status;           /* written                                               */
} VdBvhBatchItem;
int vd_bvh_build_batch(VdCtx* ctx, VdBvhBatchItem* items, uint32_t n_items, VdBvhNode* packed_nodes,
                       uint64_t packed_cap, uint32_t packed_first, uint32_t* out_packed_end);
int vd_bvh_build_batch_dev(VdCtx* ctx, VdBvhBatchItem* items, uint32_t n_items, VdBvhNode* d_packed_nodes,
                           uint64_t packed_cap, uint32_t packed_first, uint32_t* out_packed_end);

/* BLAS refit (NEW, not in the reference): new boxes for a mesh whose VERTICES moved - skinning, morph targets, cloth -
 * without a rebuild.  The topology (left_first, count) and the index buffer as the build permuted it are kept; every
 * node's min / max is recomputed.  Every box BvhBuilder writes is `calculate_bounds` over the vertices of the node's
 * triangles (blas.rs:184-204): a fold from (+1e30, -1e30) with f32::min / max, which ignore a NaN operand (tie rule
 * -0 < +0).  That min / max is associative and commutative, so an interior box is the union of its children's boxes and
 *     refit(build(x), x) == build(x)  bit for bit;
 * after a deformation the tree is the one build(x_old) chose with exact boxes for x_new (valid for every walk here; its
 * SAH quality is the old split's - rebuild when it has degraded; no heuristic for that is offered).
 * REWRITTEN: min / max of node 0 and of every node reachable from it; min / max of *mesh_info when an item carries one.
 * NOT rewritten: left_first, count, the reserved all-zero node 1 (unless a tree refers to it), every byte past n_nodes,
 * the indices, every other field of the VdMeshInfo.
 *   mesh_info   optional.  Its min / max become what MeshPool::calculate_bounds gives (crates/pools/src/mesh/mod.rs:22-27):
 *               the fold over ALL n_vert vertices from (+inf, -inf), NaN ignored - NOT the root box, which starts from
 *               +-1e30 and sees referenced vertices only.  vd_tlas_refit_dev and the cull read these bounds.
 *   packed      a mesh packed into a shared node buffer (vd_bvh_build_batch*) is an item whose `nodes` points at its
 *               out_first_node; node ids stay mesh-local.
 * vd_bvh_refit_plan_dev      once per topology.  BLOCKS (it copies nodes and indices to the host and validates them, as
 *                            vd_trace_prepare_dev validates) and derives a parent id and an arrival counter per node and
 *                            the list of leaves.  The plan keeps the items' POINTERS, not their data: vertices may change
 *                            freely, nodes' topology and indices may not.  VD_ERR_INVALID_ARG with items[m].status set
 *                            (no plan is returned) for: an interior node whose children left_first, left_first + 1 are not
 *                            both in (own id, n_nodes); a node with two parents, or a node other than 0 and the reserved
 *                            slot 1 with none; a leaf whose range [left_first, left_first + count) leaves [0, n_tri); an
 *                            index >= n_vert; n_nodes < 1; a null pointer.  Leaves may hold any number of triangles.
 *                            n_items == 0 is VD_OK: a plan that does nothing.
 * vd_bvh_refit_planned_dev   ENQUEUES ONE kernel for all items on the context's stream and nothing else - no host read,
 *                            allocation or memset - so it can be captured into a HIP graph and replayed.  A lane takes a
 *                            leaf, folds its box and climbs; at each parent the first arriver leaves, the second stores
 *                            the union and goes on.  No lane waits on another (no spin, no look-back); the counters are
 *                            back at 0 when the kernel ends, so nothing is cleared between refits.  One refit of a plan at
 *                            a time (calls on one stream are ordered).
 * vd_bvh_refit_plan_release  synchronises the stream first (a queued refit reads the plan).
 * vd_bvh_refit               host pointers, one mesh, synchronous: stage, plan, refit, copy the nodes back.
 * Per-frame order for a deforming mesh: INTEGRATION.md.  Measured against the rebuild: profiles/blas_refit.md.          */
typedef struct VdBvhRefitItem {
    const float*    verts_xyz;   /* n_vert * 3, read at every refit                      */
    const uint32_t* indices;     /* n_tri * 3, as the build permuted them; never written */
    VdBvhNode*      nodes;       /* n_nodes; only min / max are rewritten                */
    VdMeshInfo*     mesh_info;   /* optional: min / max rewritten (mesh/mod.rs:22-27)    */
    uint32_t        n_vert, n_tri, n_nodes;
    int32_t         status;      /* written by the plan call                             */
} VdBvhRefitItem;
typedef struct VdBvhRefitPlan VdBvhRefitPlan;
int vd_bvh_refit_plan_dev(VdCtx* ctx, VdBvhRefitItem* items /* host array, device pointers inside */, uint32_t n_items,
                          VdBvhRefitPlan** out);
int vd_bvh_refit_planned_dev(VdCtx* ctx, const VdBvhRefitPlan* plan);
int vd_bvh_refit_plan_release(VdCtx* ctx, VdBvhRefitPlan* plan);
int vd_bvh_refit(VdCtx* ctx, const float* verts_xyz, uint32_t n_vert, const uint32_t* indices, uint32_t n_tri,
                 VdBvhNode* nodes_inout, uint32_t n_nodes);

/* ------------------------------------------------------------------------------------ */
/* TLAS build / refit                                               */
/* ------------------------------------------------------------------------------------ */
/* Replaces `Tlas::build(&mut self, &[Instance], &[MeshInfo])`
 * (crates/bvh/src/tlas.rs:31-105), called from MeshPool::generate_tlas
 * (crates/pools/src/mesh/mod.rs:279-286). out_nodes holds 2*n+1 nodes.
 * n > 32768 => VD_ERR_TLAS_OVERFLOW (use the *_wide variant).  The *_dev forms only enqueue
 * work (from 12288 instances on the chain is shared by 16 workgroups; whether they stayed in
 * step, and the redo on one workgroup if not, is decided on the device).                  */
int vd_tlas_build(VdCtx* ctx, const VdInstance* instances, uint32_t n,
                  const VdMeshInfo* meshes, uint32_t n_mesh, VdTlasNode* out_nodes);
int vd_tlas_build_dev(VdCtx* ctx, const VdInstance* d_instances, uint32_t n,
                      const VdMeshInfo* d_meshes, uint32_t n_mesh, VdTlasNode* d_out_nodes);
int vd_tlas_build_wide(VdCtx* ctx, const VdInstance* instances, uint32_t n,
                       const VdMeshInfo* meshes, uint32_t n_mesh, VdTlasNodeWide* out_nodes);
int vd_tlas_build_wide_dev(VdCtx* ctx, const VdInstance* d_instances, uint32_t n,
                           const VdMeshInfo* d_meshes, uint32_t n_mesh,
                           VdTlasNodeWide* d_out_nodes);

/* T3 refit (NEW, not in the reference): keep the topology in nodes_inout, recompute leaf
 * boxes (tlas.rs:34-54) and interior boxes bottom-up (ascending k = n+1..2n, then
 * nodes[0] = nodes[2n]).  refit(build(x), x) == build(x) bit for bit.                   */
int vd_tlas_refit(VdCtx* ctx, const VdInstance* instances, uint32_t n,
                  const VdMeshInfo* meshes, uint32_t n_mesh, VdTlasNode* nodes_inout);
int vd_tlas_refit_dev(VdCtx* ctx, const VdInstance* d_instances, uint32_t n,
                      const VdMeshInfo* d_meshes, uint32_t n_mesh, VdTlasNode* d_nodes_inout);
int vd_tlas_refit_wide_dev(VdCtx* ctx, const VdInstance* d_instances, uint32_t n,
                           const VdMeshInfo* d_meshes, uint32_t n_mesh,
                           VdTlasNodeWide* d_nodes_inout);

/* LBVH top level (NEW, not in the reference): a top level over the reference's LEAF boxes (tlas.rs:34-54, the boxes
 * vd_tlas_build* writes) that is built on all CUs in a fraction of a millisecond, so it can be REBUILT every frame where the
 * exact builder - the reference's sequential chain - takes hundreds of milliseconds.  Not the reference's tree: what a ray
 * hits does not depend on the top level's shape except where two instances tie in distance.
 * Codes: 30-bit Morton code of the leaf-box centre (10 bits per axis) in the extent of all FINITE centres; a centre with a
 * non-finite coordinate gets the code 0x3fffffff (it sorts last; its box still folds in with the NaN-ignoring union).  Equal
 * codes are told apart by their position after the stable sort, so the tree depends on the input alone: two builds of the
 * same instances give the same bytes.  Boxes fold bottom-up with the union the refit uses (a NaN operand is ignored).
 * Node array, 2n + 1 slots, shaped like the reference's so that vd_tlas_refit[_wide]_dev takes it as it is:
 *   1 + j        the leaf of the j-th instance in sorted code order (instance_idx says which instance);
 *   n+1 .. 2n-2  the interior nodes below the root;
 *   2n - 1       the TRUE root (n >= 2);
 *   2n           {left = right = 2n - 1} with the root's box: the reference's closing self-merge (tlas.rs:59);
 *   0            a copy of node 2n - 1 - not of 2n - so a ray that misses everything walks the tree once.
 *   n == 1:      node 1 the leaf, node 2 = {left = right = 1}, node 0 a copy of the leaf.
 * The *_dev forms only enqueue: no host read-back, and no allocation once the context's work memory has reached the size
 * (one warm-up call at the largest n), so a build can be captured into a HIP graph and replayed.
 * n > VD_TLAS_MAX_INSTANCES (narrow) => VD_ERR_TLAS_OVERFLOW; n > VD_TLAS_WIDE_MAX_INSTANCES (wide) => VD_ERR_INVALID_ARG.   */
int vd_tlas_build_lbvh(VdCtx* ctx, const VdInstance* instances, uint32_t n,
                       const VdMeshInfo* meshes, uint32_t n_mesh, VdTlasNode* out_nodes /* 2n+1 */);
int vd_tlas_build_lbvh_dev(VdCtx* ctx, const VdInstance* d_instances, uint32_t n,
                           const VdMeshInfo* d_meshes, uint32_t n_mesh, VdTlasNode* d_out_nodes /* 2n+1 */);
int vd_tlas_build_lbvh_wide(VdCtx* ctx, const VdInstance* instances, uint32_t n,
                            const VdMeshInfo* meshes, uint32_t n_mesh, VdTlasNodeWide* out_nodes /* 2n+1 */);
int vd_tlas_build_lbvh_wide_dev(VdCtx* ctx, const VdInstance* d_instances, uint32_t n,
                                const VdMeshInfo* d_meshes, uint32_t n_mesh, VdTlasNodeWide* d_out_nodes /* 2n+1 */);

/* ------------------------------------------------------------------------------------ */
/* Traversal                                                           */
/* ------------------------------------------------------------------------------------ */
/* The scene the trace bind group exposes (crates/app/src/app.rs:255-287): six storage
 * buffers.  All device pointers for *_dev, all host pointers otherwise.                 */
typedef struct VdTraceScene {
    const VdTlasNode* tlas_nodes;   uint32_t n_tlas_nodes;
    const VdInstance* instances;    uint32_t n_instances;
    const VdMeshInfo* meshes;       uint32_t n_meshes;
    const VdBvhNode*  bvh_nodes;    uint32_t n_bvh_nodes;
    const float*      vertices;     uint32_t n_vertices;   /* xyz triples            */
    const uint32_t*   indices;      uint32_t n_indices;    /* reordered, all meshes  */
} VdTraceScene;

/* Replaces `traverse_tlas(ray)` (shaders/utils/bvh.wgsl:89-123) for a batch of rays.
 * out[i].dist matches the WGSL result within 1e-5 relative; a ray has 128 stack entries
 * for its TLAS + BLAS walk in registers / LDS, pushing far children only (reference: 24 per
 * walk, unchecked).  The call is TOTAL: a ray that needs more is walked again, from its start,
 * by a second pass whose stack goes on in global memory (grow-only scratch of the context,
 * allocated when first needed: 1 Ki entries per lane, then 4 Ki, ... under a 256 MB budget) -
 * same visits, same arithmetic, same record as an unbounded stack gives; calls without such a
 * ray pay nothing.  VD_ERR_STACK_OVERFLOW is left for a stack deeper than 128 + 4 Mi entries or than
 * the scene has nodes (cyclic node arrays).  BLAS leaves hold at most 3 triangles
 * (what BvhBuilder makes, blas.rs:108); anything else is VD_ERR_INVALID_ARG, and so is a TLAS
 * leaf a ray ENTERS whose instance index, whose mesh's BLAS root or whose root's children lie
 * outside the scene's buffers (unreachable slots of the TLAS array may hold anything).  Every
 * call first re-lays what the walk reads at a TLAS step and at an instance entry into one
 * cache line each (<= 65 536 TLAS nodes: a few microseconds, in the context's scratch), from
 * the scene's own buffers - nothing is cached across calls.                                   */
int vd_trace(VdCtx* ctx, const VdTraceScene* scene, const VdRay* rays, uint32_t n_rays,
             VdHit* out);
int vd_trace_dev(VdCtx* ctx, const VdTraceScene* d_scene /* struct on host, pointers on device */,
                 const VdRay* d_rays, uint32_t n_rays, VdHit* d_out);

/* The same walk over a WIDE top level (VdTlasNodeWide: 32-bit child ids, more than 32 768 instances).  The record of every
 * ray is what `traverse_tlas` (bvh.wgsl:89-123) returns when its child ids are 32 bits wide: same visits, near child first,
 * the far child pushed on `<` in the TLAS loop and on `<=` in the BLAS loop, same arithmetic - so a narrow scene whose nodes
 * are rewritten as wide ones (left = left_right & 0xffff, right = left_right >> 16), at any indices, gives the records of
 * vd_trace_dev bit for bit.  Node 0 is the root; a node with left == 0 && right == 0 is a leaf; the array may be ANY
 * arrangement (leaves need not sit at 1..n) and unreachable slots may hold anything.  VD_ERR_INVALID_ARG for a node a ray
 * REACHES with a child index >= n_tlas_nodes or, being interior, with left == 0; for everything vd_trace_dev refuses; and,
 * before anything is launched, for n_tlas_nodes > 2 * VD_TLAS_WIDE_MAX_INSTANCES + 1.  Total like the narrow call (second
 * pass over a global-memory stack, same limits), same fan-out rule, same per-call de-indexing of the leaves.  Every call
 * first writes one 64-byte record per top-level node - 48 B read, 64 B written, nothing filled: 235 MB at 2 Mi nodes - into an arena of the
 * context that only wide calls use, so narrow and wide calls may alternate.  vd_trace_prepare_wide_dev (below) makes a
 * prepared wide scene (VdTraceAccel), with VD_OPT_TRACE_TIGHT_TLAS a private tight top level for it.                   */
typedef struct VdTraceSceneWide {
    const VdTlasNodeWide* tlas_nodes; uint32_t n_tlas_nodes;
    const VdInstance* instances;    uint32_t n_instances;
    const VdMeshInfo* meshes;       uint32_t n_meshes;
    const VdBvhNode*  bvh_nodes;    uint32_t n_bvh_nodes;
    const float*      vertices;     uint32_t n_vertices;
    const uint32_t*   indices;      uint32_t n_indices;
} VdTraceSceneWide;
int vd_trace_wide(VdCtx* ctx, const VdTraceSceneWide* scene, const VdRay* rays, uint32_t n_rays, VdHit* out);
int vd_trace_wide_dev(VdCtx* ctx, const VdTraceSceneWide* d_scene /* struct on host, pointers on device */,
                      const VdRay* d_rays, uint32_t n_rays, VdHit* d_out);
int vd_trace_any_wide_dev(VdCtx* ctx, const VdTraceSceneWide* d_scene, const VdRay* d_rays, uint32_t n_rays,
                          uint32_t* d_out_hit);

/* Per-scene preparation for many trace calls over static geometry (the reference binds the six
 * buffers once per scene: app.rs:255-287): the leaf triangles are written out de-indexed, 36 bytes
 * per triangle in index-buffer (= leaf) order, so that a BLAS leaf is ONE contiguous fetch instead
 * of indices[] -> vertices[] (bvh.wgsl:30-33, 49-53).  Same vertices, same arithmetic: results are
 * bit-identical to vd_trace_dev / vd_trace_any_dev.  The accel holds a copy of the scene struct
 * (the pointers, not the data): rebuild it when indices / meshes change; after the VERTICES changed
 * (and the BLAS was refitted: vd_bvh_refit_planned_dev) vd_trace_accel_update_geometry_dev refreshes the
 * triangle copy; instances and TLAS nodes may change freely (they are read through the scene's pointers).
 * vd_trace_prepare_dev blocks (it validates the index ranges); release with vd_trace_release.  */
typedef struct VdTraceAccel VdTraceAccel;
int vd_trace_prepare_dev(VdCtx* ctx, const VdTraceScene* d_scene, VdTraceAccel** out);
int vd_trace_release(VdCtx* ctx, VdTraceAccel* accel);
/* What a prepared scene holds: whether it walks a private top level (VD_OPT_TRACE_TIGHT_TLAS was set when it was
 * prepared and every instance qualified), the nodes of the top level it walks (device pointer: the scene's own or
 * the private one), how many instances did NOT qualify (inv_transform not the inverse of transform, or non-finite
 * corners: any makes the option decline), and the bytes of de-indexed triangles it owns.                          */
typedef struct VdTraceAccelInfo {
    uint32_t tight_tlas /* 0: the scene's own top level is walked; 1 / 2: the private one, by builder */, n_tlas_nodes, tight_fallback_instances, _pad;
    uint64_t triangle_bytes;
    const VdTlasNode* d_tlas_nodes;
} VdTraceAccelInfo;
int vd_trace_accel_info(const VdTraceAccel* accel, VdTraceAccelInfo* out);
/* Rebuilds the private top level of a prepared scene from the scene's instance buffer as it is NOW (the instances moved:
 * shaders/compute_update.wgsl:10-28).  The triangles are not touched.  Blocks (it reads back whether every instance still
 * qualifies; if one does not, the walk goes back to the scene's own top level until an update finds all qualifying again).
 * A no-op for a scene prepared without VD_OPT_TRACE_TIGHT_TLAS: that one walks the host's top level, which the host refits.
 * The cheap form that keeps the tree is vd_trace_accel_refit_dev (below).                                                    */
int vd_trace_accel_update_dev(VdCtx* ctx, VdTraceAccel* accel);
/* Re-runs the de-indexing of vd_trace_prepare_dev into the accel's existing triangle array, from the scene's vertex buffer
 * as it is NOW (a mesh deformed).  Enqueues only: no validation and no read-back - indices and meshes have not changed and
 * prepare validated them - so it can be captured into a HIP graph.  The BLAS boxes are the caller's: refit them first.    */
int vd_trace_accel_update_geometry_dev(VdCtx* ctx, VdTraceAccel* accel);
int vd_trace_prepared_dev(VdCtx* ctx, const VdTraceAccel* accel, const VdRay* d_rays, uint32_t n_rays, VdHit* d_out);
int vd_trace_any_prepared_dev(VdCtx* ctx, const VdTraceAccel* accel, const VdRay* d_rays, uint32_t n_rays,
                              uint32_t* d_out_hit);

/* The prepared form of a WIDE scene: ONE handle type - the VdTraceAccel this returns is what vd_trace_prepared_dev,
 * vd_trace_any_prepared_dev, vd_trace_accel_update_dev, vd_trace_accel_refit_dev, vd_trace_accel_update_geometry_dev and
 * vd_trace_release take, and they dispatch on the handle (one made by vd_trace_prepare_dev behaves as it always did).
 * Validates as vd_trace_prepare_dev does and BLOCKS: index ranges are checked; VD_ERR_INVALID_ARG for an incomplete scene and
 * for n_tlas_nodes > 2 * VD_TLAS_WIDE_MAX_INSTANCES + 1; VD_ERR_OOM with nothing left allocated.  All leaves are de-indexed,
 * 36 B per triangle, whatever their number (the per-call de-indexing of vd_trace_wide_dev stops at 2 Mi / 16 Mi triangles).
 * Owns: the triangle copy and, when it has one, the private top level and its work memory; the six scene buffers stay the
 * caller's and must outlive the handle (the accel keeps the pointers, not the data).
 * VD_OPT_TRACE_TIGHT_TLAS == 0: the accel walks the scene's own wide nodes, read through the scene's pointers by every call -
 * they may change freely - and the records are those of vd_trace_wide_dev bit for bit.
 * VD_OPT_TRACE_TIGHT_TLAS != 0 and 2 <= n_instances <= VD_TLAS_WIDE_MAX_INSTANCES (else ignored, silently, as the narrow call
 * does): the accel owns a private VdTlasNodeWide top level over the tight boxes of VD_OPT_TRACE_TIGHT_TLAS - same rule, same
 * padding, same test of inv_transform and of finiteness - built by the LBVH builder for BOTH option values (the agglomerative
 * chain takes seconds at these sizes): tight_tlas reports 2 and 2n nodes are walked.  One instance that does not qualify and
 * the accel walks the scene's own top level (tight_fallback_instances counts them) until an update or a refit finds every
 * instance qualifying again.  Same guarantee as the narrow option: hit flags are the scene's own, distances within 1e-5, which
 * of two triangles at the same distance is reported may differ.
 * Memory held with a private top level of n instances: (2n + 1) * 48 B of nodes + 24n B of boxes + the LBVH's work memory
 * (~36n B: two key and two value arrays, links, arrival words, the sort's table) + 36 B per triangle; the first
 * vd_trace_accel_refit_dev adds 20 B per node of links and arrival words.
 * A tight accel is a SNAPSHOT of the instances: after they moved it must be updated or refitted before it is traced.          */
int vd_trace_prepare_wide_dev(VdCtx* ctx, const VdTraceSceneWide* d_scene, VdTraceAccel** out);
/* Refits the private top level of a prepared scene - narrow (either builder) or wide - to the scene's instance buffer as it is
 * NOW: new tight boxes into the leaves of the tree as it stands, then the boxes bottom-up; the TOPOLOGY is kept, so the
 * tree gets worse as the instances drift from where they were when it was built - refit per frame, vd_trace_accel_update_dev
 * (the rebuild) when the walk has slowed down.  0.03 - 0.25 ms where a rebuild takes 8.6 ms (LBVH, 1 Mi instances) or 182 ms
 * (agglomerative, 32 768).  BLOCKS like the update (it reads back whether every instance still qualifies; the decline rule
 * and the way back are the update's).  The links and arrival words of the refit live in the accel (allocated by the first
 * refit), not in the context: the caller's own vd_tlas_refit_dev at another n disturbs nothing.  VdTraceAccelInfoWide::
 * refits_since_build counts refits; an update resets it.  An agglomerative tree that was BUILT while some instance did not
 * qualify is rebuilt instead (its chain may have dropped a cluster).  A no-op returning VD_OK without a private top level.   */
int vd_trace_accel_refit_dev(VdCtx* ctx, VdTraceAccel* accel);
/* vd_trace_accel_info for a handle made by vd_trace_prepare_wide_dev.  Each of the two answers VD_ERR_INVALID_ARG for a handle
 * of the other kind, with a message that names the other function (vd_last_error of the context that prepared the handle).  */
typedef struct VdTraceAccelInfoWide {
    uint32_t tight_tlas /* 0: the scene's own top level is walked; 2: the private LBVH */, n_tlas_nodes, tight_fallback_instances, refits_since_build;
    uint64_t triangle_bytes;
    const VdTlasNodeWide* d_tlas_nodes;
} VdTraceAccelInfoWide;
int vd_trace_accel_info_wide(const VdTraceAccel* accel, VdTraceAccelInfoWide* out);

/* Occlusion query: d_out_hit[i] = traverse_tlas(ray i).hit, which is all the
 * reference's shadow pass reads (src/bin/raytraced_shadows.wgsl:97-102).  Same walk as vd_trace
 * up to the first accepted triangle, where the lane stops; the flag equals vd_trace's `hit`.  */
int vd_trace_any_dev(VdCtx* ctx, const VdTraceScene* d_scene, const VdRay* d_rays, uint32_t n_rays,
                     uint32_t* d_out_hit);
/* The shadow rays of that pass for one point light: eye = pos + nor * 0.0001, dir = light - pos
 * (not normalised; raytraced_shadows.wgsl:90-97).  positions / normals: n_points x 3 floats,
 * device; light_position: 3 floats, host.                                                  */
int vd_shadow_rays_dev(VdCtx* ctx, const float* d_positions, const float* d_normals, uint32_t n_points,
                       const float* light_position, VdRay* d_rays);

/* The CPU harness of the reference, batched on the device.
 * vd_primary_rays_dev: one ray per pixel from camera->clip_to_world, as src/bin/bvh_cpu.rs:71-83
 * builds them (pixel i: x = (i % width) / width, y = (i / height) / height - the source's own
 * row formula; eye = unprojected (x, y, 1), dir = normalised unprojected (x, y, 0)).  camera on
 * the host, d_rays: width * height rays, device.  The fragment-shader harness
 * (src/bin/bvh_trace.wgsl:225-234) makes the same rays from interpolated uv.
 * vd_traverse_iter_dev: `Bvh::traverse_iter` (crates/bvh/src/blas.rs:247-295) for every ray
 * against ONE mesh (mesh-local node ids, no TLAS): slab test dividing by dir
 * (intersection.rs:47-55), two-sided triangle test with EPS 1e-4 (intersection.rs:68-92),
 * near child pushed first.  d_out_dist[i] = closest t, or -1 for Dist::Miss.  The reference's
 * 32-entry stack panics when it overflows (blas.rs:298-324); here 128 entries and
 * VD_ERR_STACK_OVERFLOW.                                                                  */
int vd_primary_rays_dev(VdCtx* ctx, const VdCameraUniform* camera /* host */, uint32_t width,
                        uint32_t height, VdRay* d_rays);
int vd_traverse_iter_dev(VdCtx* ctx, const VdBvhNode* d_nodes, uint32_t n_nodes,
                         const float* d_verts_xyz, const uint32_t* d_indices,
                         const VdRay* d_rays, uint32_t n_rays, float* d_out_dist);
/* vd_traverse_dev: `Bvh::traverse` (crates/bvh/src/blas.rs:211-245), the reference's RECURSIVE
 * walk (its one call, `self.bvh.traverse(.., ray, 0, 1e30)`, is commented out at
 * src/bin/bvh_cpu.rs:86), for every ray against one mesh, started at node 0 with `t = t0`: same
 * slab and triangle tests as traverse_iter, children visited left then right without ordering,
 * the running t handed from call to call.  d_out_dist[i] = the returned Hit(t) - which is t0
 * itself when the ray enters the root box and hits nothing (the reference's quirk, kept) - or
 * -1 for Dist::Miss (root box missed).  The recursion is run with an explicit stack of pending
 * right children: 128 entries, VD_ERR_STACK_OVERFLOW beyond.  (The reference passes Vec4 / UVec4
 * arrays there and uses xyz; here the Vec3 / UVec3 arrays of traverse_iter.)                 */
int vd_traverse_dev(VdCtx* ctx, const VdBvhNode* d_nodes, uint32_t n_nodes,
                    const float* d_verts_xyz, const uint32_t* d_indices,
                    const VdRay* d_rays, uint32_t n_rays, float t0, float* d_out_dist);
/* host-pointer forms (staged through the context, synchronous)                            */
int vd_primary_rays(VdCtx* ctx, const VdCameraUniform* camera, uint32_t width, uint32_t height,
                    VdRay* rays);
int vd_traverse_iter(VdCtx* ctx, const VdBvhNode* nodes, uint32_t n_nodes, const float* verts_xyz,
                     uint32_t n_vert, const uint32_t* indices /* 3 * n_tri, as vd_bvh_build left them */,
                     uint32_t n_tri, const VdRay* rays, uint32_t n_rays, float* out_dist);
int vd_traverse(VdCtx* ctx, const VdBvhNode* nodes, uint32_t n_nodes, const float* verts_xyz,
                uint32_t n_vert, const uint32_t* indices, uint32_t n_tri, const VdRay* rays,
                uint32_t n_rays, float t0, float* out_dist);

/* ------------------------------------------------------------------------------------ */
/* Multi-GPU exchange over RCCL  (NEW; SURVEY.md §8e, BASELINE.json configs[3])          */
/* ------------------------------------------------------------------------------------ */
/* The reference is single-GPU (one wgpu::Device, crates/app/src/app.rs:108-118); this is the
 * north-star extension: instances shard by contiguous ranges - rank r of `world` owns
 * [r*S, min(N, (r+1)*S)), S = ceil(N / world) - and every rank ends a step with the ordered
 * compacted draw list of the WHOLE scene, bit-identical to vd_cull_compact on one GPU.  One
 * process (or thread) per GPU, one VdDist per VdCtx; the collectives are enqueued on the
 * context's stream between the two kernels, so a step is three enqueues on one stream.
 *
 *   vd_dist_unique_id       rank 0 makes the 128-byte communicator id (ncclGetUniqueId) and hands it to
 *                           the other ranks by whatever channel the host has (the Rust host: its own
 *                           IPC; the tests: a gloo broadcast).
 *   vd_dist_create          ncclCommInitRank on ctx's device; collective over all ranks.  world = 1 is a
 *                           valid communicator (a one-GPU functional check of the whole path).
 *   vd_dist_set_scene_dev   per scene: sizes the shard, builds this rank's rows of the replicated
 *                           instance -> mesh table (min(instance.mesh, n_mesh - 1); 1, 2 or 4 bytes by
 *                           table size) and all-gathers the table.  n_local must be this rank's shard
 *                           size.  Mesh assignment is static in the reference's scenes (only transforms
 *                           animate: shaders/compute_update.wgsl:10-28); call again when it changes.
 *   vd_dist_step_full_dev   vd_cull_mask_dev(own shard) -> ncclAllGather(1 bit per instance) ->
 *                           vd_expand_mask_dev(all shards): d_out[0..*d_out_count) = the whole scene's
 *                           list (d_out holds n_total commands).  No host round trip, no allocation.
 *   vd_dist_step_draws_dev  the literal exchange of the 20-byte commands: compact the own shard, all-gather
 *                           the counts (read back on the host: the sizes are data dependent), exact-size
 *                           grouped ncclSend / ncclRecv straight into every peer's final buffer.
 *   vd_dist_step_indices_dev  the same exchange with 4-byte survivor indices on the wire (SURVEY.md §8e's option;
 *                           5x fewer bytes than the commands, fewer than the bitmask when < 1 in 32 survives):
 *                           vd_cull_mask_dev -> vd_mask_to_indices_dev (global indices) -> counts (host read
 *                           back) -> grouped ncclSend / ncclRecv -> vd_indices_to_draws_dev.  Its two index
 *                           buffers (4 B per shard slot + 4 B per scene slot) are allocated on first use.
 *   vd_dist_allgather_dev   plain byte all-gather on the ctx stream (d_recv holds world * bytes_per_rank).
 * All three steps leave the same bytes in d_out[0..*d_out_count) on every rank: vd_cull_compact of the
 * whole scene.  A failed ncclSend / ncclRecv closes its group before VD_ERR_COMM is returned, so the
 * communicator's thread is never left with an open group.
 * RCCL is bound at run time: $VD_RCCL_LIB if the host sets it (an explicit choice wins - the tests bind
 * their test double this way), else the copy already loaded in the process, else librccl.so.1 /
 * /opt/rocm/lib; failure is VD_ERR_COMM, never an abort.                                             */
#define VD_DIST_ID_BYTES 128
typedef struct VdDist VdDist;
typedef struct VdDistInfo {
    int32_t  rank, world;
    uint32_t n_total, shard_size, first_instance, n_local;
    uint32_t mask_words_per_shard, id_bytes;
    uint64_t* d_mask;        /* this rank's mask (mask_words_per_shard words)                  */
    uint64_t* d_mask_all;    /* all shards' masks after a full step                            */
    void*     d_mesh_ids;    /* replicated instance -> mesh table (shard_size * world rows)    */
    int32_t  rccl_version;   /* ncclGetVersion, e.g. 22606                                     */
    int32_t  _pad;
    char     rccl_library[128];
} VdDistInfo;
int vd_dist_unique_id(void* out_id /* VD_DIST_ID_BYTES */);
int vd_dist_create(VdCtx* ctx, const void* unique_id /* VD_DIST_ID_BYTES */, int rank, int world, VdDist** out);
int vd_dist_destroy(VdDist* dist);
int vd_dist_info(const VdDist* dist, VdDistInfo* out);
int vd_dist_set_scene_dev(VdDist* dist, const VdInstance* d_shard_instances, uint32_t n_local, uint32_t n_total,
                          uint32_t n_mesh);
int vd_dist_step_full_dev(VdDist* dist, const VdCameraUniform* camera /* host */, const VdMeshInfo* d_meshes,
                          uint32_t n_mesh, const VdInstance* d_shard_instances, VdDrawIndexedIndirect* d_out,
                          uint32_t* d_out_count);
int vd_dist_step_draws_dev(VdDist* dist, const VdCameraUniform* camera /* host */, const VdMeshInfo* d_meshes,
                           uint32_t n_mesh, const VdInstance* d_shard_instances, VdDrawIndexedIndirect* d_out,
                           uint32_t* d_out_count);
int vd_dist_step_indices_dev(VdDist* dist, const VdCameraUniform* camera /* host */, const VdMeshInfo* d_meshes,
                             uint32_t n_mesh, const VdInstance* d_shard_instances, VdDrawIndexedIndirect* d_out,
                             uint32_t* d_out_count);
int vd_dist_allgather_dev(VdDist* dist, const void* d_send, void* d_recv, uint64_t bytes_per_rank);

/* ------------------------------------------------------------------------------------ */
/* Occlusion culling  (SURVEY.md §8a C4 / §8f N4 — EXTENSION, no reference counterpart)     */
/* ------------------------------------------------------------------------------------ */
/* voidin has no occlusion culling: its README (README.md:33) only links "Two-Pass Occlusion
 * Culling".  These entry points are the building blocks of that scheme on top of the cull
 * path, defined here and nowhere else; they are OFF in every parity run: no vd_cull_* call of the
 * sections above reaches them, and vd_cull_compact_hiz*, vd_cull_early_dev and vd_cull_late_dev below
 * are the extension's own.  All device pointers (vd_cull_compact_hiz takes host pointers).
 *
 * Depth convention: the reference's camera (perspective_infinite_reverse_rh, camera.rs:130-148):
 * right-handed view space looking down -z, reverse Z — depth = ndc z, 1 at the near plane, 0 at
 * infinity, cleared to 0; GREATER is nearer.  projection[11] must be -1 and projection[15] 0.
 *
 * Pyramid: level 0 = the depth buffer (width x height, row-major, row 0 = top = ndc y +1);
 * level k texel (x, y) = MIN (= farthest) of the level k-1 texels (2x..2x+1, 2y..2y+1) that
 * exist; level dims halve rounding up until 1 x 1.  vd_hiz_layout gives sizes and offsets
 * (host only, no context); the pyramid buffer holds total_texels floats.
 *
 * vd_occlusion_mask_dev: mask_out = mask_in with the bit of every OCCLUDED instance cleared
 * (bit i of word i/64 = instance i, as vd_cull_mask_dev writes them; in-place allowed).
 * Instance i is occluded when all of this holds, in fp32, in this order, no FMA:
 *   c  = ((view * transform) * vec4((mesh.min + mesh.max) / 2, 1)).xyz      (as emit_draws.wgsl:14-15)
 *   r  = length(mesh.max - mesh.min) * 0.5 * max_scale(transform)  — a TRUE bounding radius
 *        (emit_draws.wgsl:19's radius is kept bug-compatible in the frustum test; it is always
 *        >= this one but usually reaches the camera, which would disable the test)
 *   d = -c.z, dn = d - r;  dn > camera.znear            (whole sphere beyond the near plane)
 *   tangent slopes of the sphere seen from the eye, per axis a in {x, y}, t = sqrt(c.a^2 + d^2 - r^2):
 *     lo = (c.a t - r d) / (d t + c.a r),  hi = (c.a t + r d) / (d t - c.a r),  both divisors > 0
 *   ndc = P[0] * slope_x - P[8],  P[5] * slope_y - P[9];  texel range = ndc -> pixels, widened by
 *     half a texel each side, clipped to the screen (entirely off screen: not occluded)
 *   level = number of bits of max(x1 - x0, y1 - y0) (so the range is <= 2 x 2 texels there)
 *   hmin = min of the four corner texels of the range at that level
 *   (P[14] - P[10] * dn) / dn  <  hmin                  (nearest point of the sphere is farther)
 * Anything NaN fails a comparison and leaves the instance visible.                          */
typedef struct VdHizLayout {
    uint32_t width, height, n_levels, total_texels;
    uint32_t level_offset[17], level_width[17], level_height[17];   /* in texels                */
} VdHizLayout;
int vd_hiz_layout(uint32_t width, uint32_t height, VdHizLayout* out);   /* width * height <= 2^30 */
int vd_hiz_build_dev(VdCtx* ctx, const float* d_depth, uint32_t width, uint32_t height,
                     float* d_pyramid);
int vd_occlusion_mask_dev(VdCtx* ctx, const VdCameraUniform* camera /* host */,
                          const VdMeshInfo* d_meshes, uint32_t n_mesh,
                          const VdInstance* d_instances, uint32_t n_inst,
                          const float* d_pyramid, uint32_t width, uint32_t height,
                          const uint64_t* d_mask_in, uint64_t* d_mask_out);

/* Occlusion-culled draw lists: the ordered list of the instances that pass the frustum test AND are not occluded, from ONE
 * read of the instances (the composition vd_cull_mask_dev -> vd_occlusion_mask_dev -> vd_expand_mask_dev reads them twice
 * and needs a caller-built mesh-id table).  Pinned by what exists.  With
 *   F = the bits vd_cull_mask_dev writes,   V = vd_occlusion_mask_dev(F),
 *   P = d_prev_visible (bit i % 64 of word i / 64 = instance i, ceil(n_inst / 64) words; padding bits are ignored):
 *   vd_cull_compact_hiz_dev   list of V, ascending instance order; the commands are the ones vd_cull_compact_dev writes
 *                             for those instances (base_instance = index).
 *   vd_cull_early_dev         first half of the two-pass scheme: list of E = F & P - what was visible last frame and
 *                             is still in the frustum.  The caller draws it, then builds the pyramid of that depth.
 *   vd_cull_late_dev          second half: list of L = V & ~P - what the new pyramid reveals - and d_visible_out = V
 *                             (padding bits 0), next frame's P.  EVERY instance of F is tested against the pyramid, E
 *                             included: an instance drawn this frame but hidden now leaves next frame's early list.
 *                             d_visible_out may be d_prev_visible (in place).  F is recomputed, so nothing but the
 *                             caller's buffers is carried from the early call; other vd_cull_* calls may run in between.
 * Hence E and L are disjoint, E | L covers V; P = 0: late == hiz and early is empty; P = all ones: early ==
 * vd_cull_compact_dev and late is empty.  pad_tail as in vd_cull_compact_dev (zeroes [count, n_inst)); without it nothing
 * behind the count is written.  Always two launches (three with pad_tail), at every size: one pass over the instances
 * that writes a bitmask, then the expansion; no scan, no wait between workgroups, hence no "gave up" state.  Like the
 * other per-frame entry points they only enqueue kernels on the context's stream once their scratch exists (first call, or
 * a larger scene), so an early -> vd_hiz_build_dev -> late frame can be captured into a HIP graph; the camera is baked
 * in by value.  vd_last_gpu_ms_stage: 0 = the pass over the instances, 1 = the expansion.
 * VD_ERR_INVALID_ARG: null ctx / camera / meshes / count, n_mesh == 0; where a pyramid is taken: null pyramid, a size
 * vd_hiz_layout refuses, a projection that is not the kind vd_occlusion_mask_dev accepts; with n_inst > 0: null
 * instances / out / visibility masks.  n_inst == 0 sets the count to 0 and touches nothing else.
 * Bytes moved and measured times: DESIGN.md 3.6, profiles/cull_occlusion.md.                                           */
int vd_cull_compact_hiz_dev(VdCtx* ctx, const VdCameraUniform* camera /* host */,
                            const VdMeshInfo* d_meshes, uint32_t n_mesh,
                            const VdInstance* d_instances, uint32_t n_inst,
                            const float* d_pyramid, uint32_t width, uint32_t height,
                            VdDrawIndexedIndirect* d_out, uint32_t* d_out_count, int pad_tail);
int vd_cull_early_dev(VdCtx* ctx, const VdCameraUniform* camera /* host */,
                      const VdMeshInfo* d_meshes, uint32_t n_mesh,
                      const VdInstance* d_instances, uint32_t n_inst,
                      const uint64_t* d_prev_visible,
                      VdDrawIndexedIndirect* d_out, uint32_t* d_out_count, int pad_tail);
int vd_cull_late_dev(VdCtx* ctx, const VdCameraUniform* camera /* host */,
                     const VdMeshInfo* d_meshes, uint32_t n_mesh,
                     const VdInstance* d_instances, uint32_t n_inst,
                     const float* d_pyramid, uint32_t width, uint32_t height,
                     const uint64_t* d_prev_visible, uint64_t* d_visible_out /* may alias d_prev_visible */,
                     VdDrawIndexedIndirect* d_out, uint32_t* d_out_count, int pad_tail);
/* host-pointer form of vd_cull_compact_hiz_dev (the pyramid too: total_texels floats), staged through the context and
 * synchronous, like vd_cull_compact                                                                                   */
int vd_cull_compact_hiz(VdCtx* ctx, const VdCameraUniform* camera,
                        const VdMeshInfo* meshes, uint32_t n_mesh,
                        const VdInstance* instances, uint32_t n_inst,
                        const float* pyramid, uint32_t width, uint32_t height,
                        VdDrawIndexedIndirect* out, uint32_t* out_count, int pad_tail);

/* ------------------------------------------------------------------------------------ */
/* Level of detail  (EXTENSION, no reference counterpart)                                   */
/* ------------------------------------------------------------------------------------ */
/* The reference draws every instance with the one index range of instances[i].mesh.  These entry points choose a level of
 * detail per instance while the cull pass has it in registers, and write the choice where the draw lists already take
 * their index ranges from: the per-instance id that the expansion (vd_expand_mask_dev) and the grouping
 * (vd_batch_mask_dev) look up in d_meshes.  They are defined here and nowhere else and are OFF in every parity run: no
 * entry point of the sections above reaches them.
 *
 * Instance.mesh indexes a table of GROUPS; a group names a run of consecutive ROWS of d_meshes, one per level, finest
 * first.  Each level is an ordinary VdMeshInfo row (what MeshPool::add produces), so the consumer is unchanged:
 * multi_draw_indexed_indirect reads index ranges as before.  Only index_count / base_index / vertex_offset of a row are
 * used; the box that is tested and measured is the group's.
 *
 * For instance i, in fp32, in this order, no FMA (n_group groups, n_mesh rows, P = the VdLodParams):
 *   g       = min(instances[i].mesh, n_group - 1),  G = groups[g]
 *   c       = ((view * transform) * vec4((G.min + G.max) / 2, 1)).xyz               (as emit_draws.wgsl:14-15)
 *   visible = the frustum test of vd_cull_emit with G.min / G.max as the mesh box    (bug-compatible radius included)
 *   r       = (length(G.max - G.min) * 0.5) * max_scale(transform)                   (the r of "Occlusion culling")
 *   d       = -c.z
 *   dist    = fmaxf(d, P.min_distance)                                               (a NaN d gives min_distance)
 *   size    = (r * P.scale) / dist
 *   nl      = clamp(G.n_lods, 1, VD_LOD_MAX)
 *   lod     = the NUMBER of k < nl - 1 with size < G.switch_size[k]    (a count, not a first failure: defined for
 *             unsorted thresholds; a NaN size gives 0, the finest level)
 *   row     = min(min(G.first_row, n_mesh - 1) + lod, n_mesh - 1)
 *   drawn   = visible && !(size < P.min_size)                                        (contribution culling; 0 = off)
 * With scale = projection[5] * viewport_height / 2, size is the projected radius of the bounding sphere in pixels.
 *
 *   vd_lod_ids_dev            d_out_ids[i] = row(i) for EVERY instance (visibility and min_size play no part), as ids of
 *                             id_bytes = 1, 2 or 4 bytes, which must be able to hold n_mesh - 1.  The table must be
 *                             16-byte aligned.  With it any mask the library produces (vd_cull_mask_dev on the groups'
 *                             boxes, vd_occlusion_mask_dev, the all-gathered masks of vd_dist_*) is expanded or grouped by
 *                             LOD row through vd_expand_mask_dev / vd_batch_mask_dev.
 *   vd_cull_compact_lod_dev   the ordered list of the instances with `drawn`: { d_meshes[row(i)].index_count, 1,
 *                             d_meshes[row(i)].base_index, d_meshes[row(i)].vertex_offset, i }, ascending i, and the
 *                             count.  pad_tail as in vd_cull_compact_dev; without it nothing behind the count is written.
 *   vd_cull_batch_lod_dev     the instanced form ("Instanced draw lists") over rows: one command per ROW of d_meshes -
 *                             one per (mesh, level) - and the drawn instances' ids grouped by row.  n_mesh <=
 *                             VD_BATCH_MAX_MESHES applies to rows.
 *   vd_cull_compact_lod       host pointers, staged through the context and synchronous, like vd_cull_compact.  It sees the
 *                             group table and refuses (VD_ERR_INVALID_ARG) one that breaks 1 <= n_lods <= VD_LOD_MAX or
 *                             first_row + n_lods <= n_mesh in any group.
 * The *_dev forms do not read the group table back: the clamps above make every table defined.
 * Always the split form, at every size: one pass over the instances (cull to bitmask + the row of every instance in the
 * id table + survivors per tile), then the unchanged expansion or grouping: two launches for the list, three with
 * pad_tail.  No atomics, no wait between workgroups, hence no "gave up" state.  The pass shares the context's id table
 * with vd_cull_compact_dev: calls of both kinds, also with different id widths, may alternate on one context - every
 * row of the table that differs from the call's is rewritten.  Once its scratch exists (first call, or a larger scene)
 * a call only enqueues kernels on the context's stream, so it can be captured into a HIP graph; the camera and the
 * parameters are baked in by value.  vd_last_gpu_ms_stage: 0 = the pass over the instances, 1 = everything after it.
 * VD_ERR_INVALID_ARG: null ctx / camera / groups / meshes / count (cmds); n_group == 0 or n_mesh == 0; scale not finite
 * or < 0; min_distance not finite or <= 0; min_size not finite or < 0; id_bytes not 1, 2 or 4 or too narrow for
 * n_mesh - 1; a misaligned id table; with n_inst > 0: null instances / out / ids.  A refused call writes nothing.
 * n_inst == 0: as in the sibling calls (the count is set to 0; vd_cull_batch_lod_dev writes its n_mesh empty commands;
 * vd_lod_ids_dev does nothing).
 * OUT OF SCOPE: hysteresis or any per-instance LOD state; cross-fade; a multi-view form; a fused occlusion + LOD form
 * and a vd_dist_* form (both are compositions of vd_lod_ids_dev with the existing mask consumers).
 * Measured times against vd_cull_compact_dev / vd_cull_batch_dev: profiles/cull_lod.md.                                 */
#define VD_LOD_MAX 8u
typedef struct VdLodGroup {          /* 64 B, 16-byte aligned rows; indexed by Instance.mesh */
    float    min[3];  uint32_t first_row;   /* box used by the visibility test and the size metric; row of LOD 0 in d_meshes */
    float    max[3];  uint32_t n_lods;      /* 1 .. VD_LOD_MAX, LOD k is row first_row + k     */
    float    switch_size[VD_LOD_MAX - 1];   /* LOD k+1.. is taken while size < switch_size[k]  */
    uint32_t _pad;
} VdLodGroup;
typedef struct VdLodParams {         /* host, by value */
    float scale;         /* e.g. projection[5] * viewport_height / 2: size = projected radius in pixels */
    float min_distance;  /* > 0, finite */
    float min_size;      /* >= 0; 0 = off; an instance with size < min_size is not drawn (contribution culling) */
    uint32_t _pad;
} VdLodParams;
int vd_lod_ids_dev(VdCtx* ctx, const VdCameraUniform* camera /* host */, VdLodParams params,
                   const VdLodGroup* d_groups, uint32_t n_group, uint32_t n_mesh,
                   const VdInstance* d_instances, uint32_t n_inst,
                   void* d_out_ids /* n_inst ids */, uint32_t id_bytes /* 1, 2, 4 */);
int vd_cull_compact_lod_dev(VdCtx* ctx, const VdCameraUniform* camera /* host */, VdLodParams params,
                            const VdLodGroup* d_groups, uint32_t n_group,
                            const VdMeshInfo* d_meshes, uint32_t n_mesh,
                            const VdInstance* d_instances, uint32_t n_inst,
                            VdDrawIndexedIndirect* d_out, uint32_t* d_out_count, int pad_tail);
int vd_cull_batch_lod_dev(VdCtx* ctx, const VdCameraUniform* camera /* host */, VdLodParams params,
                          const VdLodGroup* d_groups, uint32_t n_group,
                          const VdMeshInfo* d_meshes, uint32_t n_mesh,
                          const VdInstance* d_instances, uint32_t n_inst,
                          VdDrawIndexedIndirect* d_out_cmds /* n_mesh */, uint32_t* d_out_instance_ids /* n_inst */,
                          uint32_t* d_out_count);
int vd_cull_compact_lod(VdCtx* ctx, const VdCameraUniform* camera, VdLodParams params,
                        const VdLodGroup* groups, uint32_t n_group,
                        const VdMeshInfo* meshes, uint32_t n_mesh,
                        const VdInstance* instances, uint32_t n_inst,
                        VdDrawIndexedIndirect* out, uint32_t* out_count, int pad_tail);

/* ------------------------------------------------------------------------------------ */
/* Ray intervals  (VD_OPT_TRACE_RAY_RANGE; no reference counterpart: its rays have no end) */
/* ------------------------------------------------------------------------------------ */
/* (This section stands behind the level-of-detail calls and not next to vd_trace*, and the notes at VdRay and at the
 * option are kept to the lines that were there: tests/stream_order_cases.py quotes lines of this header by number.)
 * vd_ctx_set_option(ctx, VD_OPT_TRACE_RAY_RANGE, 1): every vd_trace* call of the context - vd_trace, vd_trace_dev,
 * vd_trace_any_dev, vd_trace_wide, vd_trace_wide_dev, vd_trace_any_wide_dev, vd_trace_prepared_dev and
 * vd_trace_any_prepared_dev, with or without a private top level (VD_OPT_TRACE_TIGHT_TLAS) - reads VdRay::_pad0 as t_min
 * and VdRay::_pad1 as t_max:
 *     t_lo = fmaxf(_pad0, 0.0f)          a NaN or negative t_min reads as 0
 *     t_hi = fminf(_pad1, VD_MAX_DIST)   a NaN or oversized t_max reads as 1e30; a negative or zero t_max stays as it
 *                                        is, and the ray misses
 * The record of a ray is what traverse_tlas (bvh.wgsl:89-123) returns when two things change: its result starts at
 * dist = t_hi instead of MAX_DIST, and intersect_trig accepts t_lo < t && t < hit instead of 0 < t && t < hit.  That is
 * the minimum over (t, visit order) of the triangles the ray truly intersects inside the OPEN interval (t_lo, t_hi) -
 * both ends are exclusive.  The arithmetic, the box tests and the pruning by the distance found so far are the same;
 * nothing is pruned by t_lo.
 *   - A miss is the miss record of the default: dist = VD_MAX_DIST, hit = 0 and the instance / triangle words a miss has
 *     without the option.  It never holds t_hi.
 *   - The any-hit flag equals the closest-hit `hit` of the same interval.
 *   - With t_lo = 0 and t_hi = VD_MAX_DIST every output is, byte for byte, the output with the option off.
 *   - t stays the parameter of the ray as given: `dir` is not normalised, inside an instance neither.  So t_max = 1 on a
 *     ray whose dir = light - origin is the light, whatever the instance scales.
 * The option is read at each call and latched by nothing (vd_trace_prepare* included): one prepared scene serves calls
 * of both kinds.  A call enqueues and blocks exactly where it does without the option - the same launches, over other
 * instantiations of the same kernels - so what could be captured into a HIP graph still can.
 * The ray generators follow the option: vd_shadow_rays_dev writes _pad0 = 0, _pad1 = 1 - the open segment from the
 * offset surface point to the light, so geometry BEHIND the light no longer shadows the point (it does in the reference,
 * raytraced_shadows.wgsl:90-102, and by default) and no box beyond the light is entered; vd_primary_rays_dev and
 * vd_primary_rays write 0 and VD_MAX_DIST.  With the option off they write 0 and 0 as before, bit for bit, and the walk
 * ignores both words whatever they hold.  The host forms copy whole 32-byte rays.  ray_segment() in voidin.hpp and
 * set_ray_range() in voidin_amd/runtime.py fill the two fields.  Measured: profiles/trace_ray_range.md.              */

/* ------------------------------------------------------------------------------------ */
/* Instance animation  (SURVEY.md §8f N2 — the upstream mutator of the cull / TLAS input)  */
/* ------------------------------------------------------------------------------------ */
/* Replaces the `update` compute pass (shaders/compute_update.wgsl:10-28, recorded by
 * ComputeUpdate::record, crates/app/src/pass/compute_update.rs:51-73): for every listed
 * instance id, transform = rotz(speed * dt) * transform with speed = 2*sin(time*0.5), negated
 * when transform[3][2] <= -15.  sin/cos are evaluated once on the host (libm, f32) for the
 * two possible angles, so the device work is plain mul/add and matches the oracle bit for bit
 * (WGSL leaves sin/cos precision to the driver).
 * fix_inverse != 0 additionally keeps inv_transform consistent (inv' = inv * rotz(-angle));
 * the reference leaves it stale.                                   */
int vd_compute_update_dev(VdCtx* ctx, const uint32_t* d_indices, uint32_t n_indices,
                          VdInstance* d_instances, uint32_t n_instances, float time, float dt,
                          int fix_inverse);

/* ------------------------------------------------------------------------------------ */
/* Instrumentation (replaces the wgpu_profiler scopes: visibility.rs:50,243-245)         */
/* ------------------------------------------------------------------------------------ */
/* Opt-in kernel timing: with timing enabled every call brackets its kernels with a HIP event
 * pair on the ctx's stream (costs a few microseconds of GPU idle per call, so it is off by
 * default).  vd_last_gpu_ms returns the milliseconds of the most recent call's kernels
 * (synchronises); negative if timing is off or nothing was recorded.                     */
int   vd_ctx_set_timing(VdCtx* ctx, int enabled);
float vd_last_gpu_ms(VdCtx* ctx);
/* For calls that run two passes (vd_cull_compact* on large inputs: cull-to-bitmask, then
 * expansion): milliseconds of pass `stage` (0 or 1); negative when the call had one pass.  */
float vd_last_gpu_ms_stage(VdCtx* ctx, int stage);
/* Where the most recent vd_bvh_build[_dev] on this ctx spent its time: host wall clock between the
 * synchronisation points the builder has anyway (after the precompute, after the level loop of the
 * large segments, after the mid tier, after the small subtrees, after copy-out + index permute).   */
typedef struct VdBvhBuildStats {
    float    ms_precompute, ms_phase_a, ms_mid, ms_phase_b, ms_phase_c;
    uint32_t levels_phase_a;      /* level-synchronous rounds over segments > 2048 prims */
    uint32_t n_top_nodes, n_mid_roots, n_small_roots;
    uint32_t kernel_launches;     /* kernels enqueued by the build */
} VdBvhBuildStats;
int vd_bvh_last_build_stats(const VdCtx* ctx, VdBvhBuildStats* out);

#ifdef __cplusplus
}
#endif
#endif /* VOIDIN_ABI_H */
