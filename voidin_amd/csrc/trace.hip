// trace.hip — batch TLAS -> instance -> BLAS ray traversal on gfx950.
//
// Replaces `traverse_tlas(ray)` (reference: shaders/utils/bvh.wgsl:89-123) and its callees
// `instance_intersect` (bvh.wgsl:78-87), `traverse_bvh` (bvh.wgsl:35-76), `fetch_vertex`
// (bvh.wgsl:30-33), `intersect_aabb` / `intersect_trig` (shaders/utils/intersections.wgsl:13-45).
// One lane per ray at a time, persistent waves that refill (see trace_body); the arithmetic order is the WGSL
// source order with no FMA, so hit distances are reproduced to the bit on the oracle's evaluation model (tolerance
// in tests: 1e-5).  The reference's 24-entry stack is unchecked (shaders/utils/stack.wgsl:1-20); here one 128-entry
// stack serves the TLAS and the BLAS walk of a ray, and a ray that needs more is walked AGAIN, from its start, by a second
// pass whose stack goes on in a slab of global memory (launch_trace: the call is total - VD_ERR_STACK_OVERFLOW is left for
// scenes whose trees are deeper than the slab the context may allocate).  Leaves of more than 3
// triangles do not occur (BvhBuilder stops at <= 3: blas.rs:108) and are not representable in a stack entry.
#include "vd_common.hpp"

#include <algorithm>
#include <cstddef>
#include <new>
#include <type_traits>

// vd_trace_prepare_dev: per-scene data derived once from the six trace buffers.  The triangle copy follows the scene's
// vertex buffer through vd_trace_accel_update_geometry_dev (a mesh deformed: same indices and meshes, new positions), which
// re-runs the de-indexing into the same array without validating or reading anything back.
// vd_trace_prepare_wide_dev makes the same handle over a VdTraceSceneWide (`wide`): the two scene structs differ in the node type
// their first pointer names and in nothing else, so the accel keeps one copy, typed by `wide` (accel_scene<WIDE>), and its node
// pointers as void*.
struct VdTraceAccel {
    union { VdTraceScene scene; VdTraceSceneWide wscene; };
    bool wide = false; float* tris = nullptr;
    // private top level (VD_OPT_TRACE_TIGHT_TLAS): its nodes, which builder made it (1 agglomerative, 2 LBVH), the scene's own top
    // level (what the walk goes back to when an update finds an instance that does not qualify), work memory of the builders
    void* tight = nullptr; unsigned tight_mode = 0, tight_fallbacks = 0;
    const void* user_tlas = nullptr; unsigned user_n_nodes = 0;
    float* boxes = nullptr; unsigned* lbvh = nullptr;
    // vd_trace_accel_refit_dev: its links and arrival words (allocated by the first refit), refits since the tree was built, and
    // how many instances did not qualify when it was BUILT (the agglomerative chain drops a cluster it finds no partner for)
    VdRefitArena refit; unsigned refits = 0, built_fallbacks = 0;
    VdCtx* owner = nullptr;      // the context that prepared it: where the info calls, which take none, leave their message
    VdTraceAccel() : scene{} {}
};
static_assert(sizeof(VdTraceScene) == sizeof(VdTraceSceneWide) && offsetof(VdTraceScene, instances) == offsetof(VdTraceSceneWide, instances) &&
              offsetof(VdTraceScene, n_indices) == offsetof(VdTraceSceneWide, n_indices), "one layout, two node types");

namespace {

constexpr int kStack = 64;
constexpr int kLdsStack = 24;            // stack entries per ray kept in LDS: 6 KB per wave, 24 waves per CU = 144 of the 160 KB
constexpr float kMaxDist = 1e30f;

struct Ray { float ex, ey, ez, dx, dy, dz, ix, iy, iz; };

__device__ __forceinline__ float min3(float a, float b, float c) { return fminf(a, fminf(b, c)); }   // math.wgsl:19-21
__device__ __forceinline__ float max3(float a, float b, float c) { return fmaxf(a, fmaxf(b, c)); }   // math.wgsl:23-25

// intersections.wgsl:13-23
__device__ __forceinline__ float intersect_aabb(const Ray& r, const float* mn, const float* mx, float t) {
    const float ax = (mn[0] - r.ex) * r.ix, ay = (mn[1] - r.ey) * r.iy, az = (mn[2] - r.ez) * r.iz;
    const float bx = (mx[0] - r.ex) * r.ix, by = (mx[1] - r.ey) * r.iy, bz = (mx[2] - r.ez) * r.iz;
    const float tmax = min3(fmaxf(ax, bx), fmaxf(ay, by), fmaxf(az, bz));
    const float tmin = max3(fminf(ax, bx), fminf(ay, by), fminf(az, bz));
    return (tmax >= tmin && tmin < t && tmax > 0.0f) ? tmin : kMaxDist;
}

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
    return (ax * bx + ay * by) + az * bz;
}

// intersections.wgsl:25-45 (Moeller-Trumbore, backface cull det < 1e-10)
// RANGE (VD_OPT_TRACE_RAY_RANGE): t is accepted above t_lo instead of above 0 - the lower end of the ray's interval, exclusive.
template <bool RANGE = false>
__device__ __forceinline__ bool intersect_trig(const Ray& r, const float* v0, const float* v1, const float* v2, float& hit, float t_lo = 0.0f) {
    const float e1x = v1[0] - v0[0], e1y = v1[1] - v0[1], e1z = v1[2] - v0[2];
    const float e2x = v2[0] - v0[0], e2y = v2[1] - v0[1], e2z = v2[2] - v0[2];
    // cross(dir, edge2)
    const float ux = r.dy * e2z - e2y * r.dz, uy = r.dz * e2x - e2z * r.dx, uz = r.dx * e2y - e2x * r.dy;
    const float det = dot3(e1x, e1y, e1z, ux, uy, uz);
    if (det < 1e-10f) return false;
    const float inv_det = 1.0f / det;
    const float ox = r.ex - v0[0], oy = r.ey - v0[1], oz = r.ez - v0[2];
    const float u = inv_det * dot3(ox, oy, oz, ux, uy, uz);
    if (u < 0.0f || 1.0f < u) return false;
    // cross(orig, edge1)
    const float vx = oy * e1z - e1y * oz, vy = oz * e1x - e1z * ox, vz = ox * e1y - e1x * oy;
    const float v = inv_det * dot3(r.dx, r.dy, r.dz, vx, vy, vz);
    if (v < 0.0f || u + v > 1.0f) return false;
    const float t = inv_det * dot3(e2x, e2y, e2z, vx, vy, vz);
    if (t > (RANGE ? t_lo : 0.0f) && t < hit) {
        hit = t;
        return true;
    }
    return false;
}

struct Scene {
    const VdTlasNode* tlas; const VdInstance* inst; const VdMeshInfo* meshes; const VdBvhNode* bvh;
    const float* verts; const unsigned* indices; unsigned n_meshes;
    const float* tris;          // vd_trace_prepare_dev: 9 floats per triangle in index-buffer order (nullptr: not prepared)
    const float4* irec;         // entry records, 4 x float4 per TLAS node (records_kernel)
    const float4* tpair;        // child pairs of the TLAS, 4 x float4 per node, at the LEFT child's index
    const float4* mrec;         // mesh records, 8 x float4 per mesh
    unsigned yield;             // waiting lanes at which a wave leaves the stepping loop (VD_OPT_TRACE_YIELD)
    unsigned* ovf_bits = nullptr;   // first pass: bit r is set when ray r ran out of its 128 entries (the second pass walks those again)
    unsigned* deep = nullptr;       // second pass (DEEP): entries 128.. of a lane's stack, [wave][entry][lane]
    unsigned deep_cap = 0;          // ... and how many there are per lane
};

// Where a wave's rays come from: idle lanes draw single positions 0 .. n_rays - 1 from the global counter `next`, and
// position p is ray order[p] (nullptr = identity: the first pass; the deep second pass hands out its overflow list).
// Handing the rays out in a sorted order or in per-workgroup chunks was tried and lost: DESIGN.md 3.5.
// Fan-out (see kFan*): one job = one TLAS subtree of one ray.  48 bytes: as a pending job {ray, the distance
// found so far, ray id, order key, the subtree as a stack-entry word}; when finished the same slot holds the job's result.
struct FanJob { float ex, ey, ez, dx, dy, dz; float lim; unsigned ray_id, key, node, state, tri; };
static_assert(sizeof(FanJob) == 48, "FanJob is three uint4");
enum : unsigned { FAN_PENDING = 0u, FAN_MISS = 1u, FAN_HIT = 2u, FAN_NULL = 3u };
struct Fan {                       // one launch's place in the fan-out (all nullptr / 0: a plain call)
    FanJob* jobs; const unsigned* begin; const unsigned* end;      // this launch's supply = jobs[*begin, *end) instead of fresh rays (end == nullptr: fresh rays)
    unsigned* append; unsigned cap;                                // where new jobs go: jobs[atomicAdd(append, n)], n <= cap
    unsigned long long* best;                                      // per ray: min over finished jobs of {distance bits, key}
    unsigned below, level;                                         // fan out when fewer than `below` rays are alive in a draining wave (0: never); key digit position
};
struct RaySource { const unsigned* order; unsigned n_rays; unsigned* next; Fan fan = {}; };

// Fan-out.  The stress scene's call is as long as its longest rays - 8 500 dependent steps of ~1.4 us against a mean of 517 -
// and for most of it a few waves each nurse a handful of such rays while the rest of the machine is idle (the "relay" that
// only repacked whole rays into full waves made it slower: profiles/r04_trace_relay_experiment.log).  A ray's remaining work
// IS its stack: every entry is a TLAS subtree still to be visited, and visits of different subtrees do not depend on each
// other except through the distance found so far.  So a call runs as a few launches: once the rays are handed out, a wave
// that is down to fewer than kFanBelow live rays turns each of them (when it is between instances: the stack then holds TLAS
// entries only) into jobs - one for the node it is at, one per stack entry - that start from the distance the ray has
// found so far, and ends; the next launch's waves draw jobs like rays, 64 per wave, and may fan out again.
// Same result, bit for bit: the walk's answer is the minimum of (t, visit order) over the triangles the ray truly
// intersects - pruning by the current distance only ever skips candidates that cannot beat it, and a later candidate at an
// equal t loses (intersections.wgsl:40 `t < hit`).  Visit order over the tree is fixed by the ray alone (near child first,
// by slab distance), so it is carried as a key: the ray's own result so far is digit 0, the node it is at digit 1, its stack
// entries top to bottom digits 2, 3, ... - one digit per launch that fanned the job out - and a job accepts only t strictly
// below the distance it started from, so an equal t never beats anything found before the fan-out.  Each finished job
// records {distance bits, key} with an atomic min per ray; vd_fan_resolve_kernel lets the job that holds the minimum write the
// ray's record.  (The reference's root is visited twice - tlas.rs:59 merges the true root with itself - and the second
// visit can only tie: its job is not created.)
constexpr unsigned kFanPhases = 3;            // launches per call (VD_OPT_TRACE_FAN; 1 = one launch, no fan-out)
constexpr unsigned kFanBelow = 32;            // live rays below which a draining wave fans its rays out at once
constexpr unsigned kFanGrace = 128;           // stepping iterations after the last draw before a wave fans out whatever is still alive
constexpr unsigned kFanAgain = 8;             // ... and between two looks at the rays that were inside an instance at the time
constexpr unsigned kFanAge = 512;             // only rays that have been stepping for at least this many of the wave's iterations fan out (0: all)

// A fixed grid of waves; a lane whose ray is finished draws the next ray from a counter, so a wave stays full while
// rays of very different cost (a few node visits to thousands) pass through it.  To let a lane restart at any point the
// TLAS walk and the per-instance BLAS walk are ONE state machine over ONE stack (TLAS and BLAS nodes share the 32-byte
// {min, u32, max, u32} layout).  Every busy lane makes ONE fetch per iteration of the stepping loop, whatever it is
// doing - an interior node's child pair, the entry record of the instance it enters, a de-indexed triangle - into one set
// of registers (see the loop).  Each ray still sees exactly the reference's sequence of node visits and triangle tests
// (bvh.wgsl:35-123); only the interleaving across lanes changes.
// ANY: occlusion query - the lane stops at the first accepted triangle and only `hit` is reported.  That flag is
// the same as the closest-hit traversal's: until something is accepted nothing is pruned by distance, so both walks
// visit the same nodes up to that point (the reference's shadow pass uses only `.hit`: raytraced_shadows.wgsl:97-102).
constexpr long long kYieldDefault = 1;   // see the stepping loop (sweep in profiles/r03_ab_trace.log: 1 is best)
constexpr unsigned kRefillBelow = 56;   // draw new rays when fewer than this many lanes are busy
constexpr unsigned kWavesPerCu = 24;    // persistent grid = what is resident (6 waves per SIMD at <= 84 VGPRs: the walk holds ~76, and with 72 it spilled): no wave starts late
// PREP: leaf triangles come de-indexed from Scene::tris (one contiguous fetch instead of indices[] -> verts[]).
// FAN: the fan-out's code is compiled in (src.fan says what this launch hands out and whether it may append jobs).
// DEEP: the second pass over the rays whose stack overflowed (launch_trace) - same walk, entries 128.. in s.deep.
// Every kernel that calls this runs one wave per workgroup.
// WIDE: the top level is an array of VdTlasNodeWide (vd_trace_wide*: 32-bit child ids), which Scene::tlas then points at.
// What differs is how a TLAS node is named.  Narrow: an interior node is its left_right word, a leaf its index << 16 - in
// a stack entry, in FanJob.node and as the current node cn = {left_right, own index}.  Wide: a node is its own INDEX, with
// bit 31 set for a leaf, and cn = {1 interior / 0 leaf, index}; the 64-byte record of an interior node sits at the node's
// own index and holds both children's boxes with their cn words (records_wide_kernel), so a step is one line as before
// and no record is shared between two parents.
// RANGE (VD_OPT_TRACE_RAY_RANGE): a ray is the open interval (t_lo, t_hi) of its line instead of (0, 1e30): t_lo = max(_pad0, 0) is
// one more per-lane value that lives through the walk (intersect_trig accepts above it), t_hi = min(_pad1, 1e30) is what res.dist
// starts from instead of kMaxDist - the pruning, the visit order and the fan-out's keys are what they were (a job's `lim` is t_hi
// until something is hit; its t_lo is read again from the ray) - and a ray that ends without a hit reports kMaxDist, not t_hi.
// (The narrow forms stay written out where they are used, behind `WIDE ? ... :` - a constant the front end folds: moved
// into functions like these, the narrow kernels came out with other register numbers.)
__device__ __forceinline__ uint2 tl_node_wide(unsigned w) { return make_uint2((w >> 31) ^ 1u, w & 0x7fffffffu); }
__device__ __forceinline__ unsigned tl_word_wide(const uint2 cn) { return cn.x != 0u ? cn.y : (cn.y | 0x80000000u); }
template <bool WIDE, typename S> __device__ __forceinline__ unsigned tl_instance(const S& s, unsigned leaf) {
    if constexpr (WIDE) return reinterpret_cast<const VdTlasNodeWide*>(s.tlas)[leaf].instance_idx;
    else return s.tlas[leaf].instance_idx;
}
template <bool ANY, bool PREP, bool FAN = false, bool DEEP = false, bool WIDE = false, bool RANGE = false>
__device__ __forceinline__ void trace_body(const Scene& s, const VdRay* __restrict__ rays, const RaySource& src, VdHit* __restrict__ out,
                                           unsigned* __restrict__ out_any, unsigned* __restrict__ overflow) {
    const unsigned lane = threadIdx.x & 63u;
    const bool from_jobs = FAN && src.fan.end != nullptr;                       // this launch hands out jobs, not fresh rays
    const unsigned job_begin = from_jobs ? *src.fan.begin : 0u;
    const unsigned n_rays = from_jobs ? *src.fan.end - job_begin : src.n_rays;     // what this launch hands out
    bool fan_off = false;                  // wave-uniform: the job list was full when this wave wanted to fan out
    unsigned drain_iters = 0;              // wave-uniform: stepping iterations since this wave found the supply empty
    unsigned wave_iters = 0;               // wave-uniform: stepping iterations of this wave (FAN: a ray's age = now - s_born[lane])
    __shared__ unsigned s_born[(FAN && kFanAge) ? 64 : 1];
    // The first kLdsStack entries of a ray's stack live in LDS ([slot][lane]: a lane always hits its own bank), the rest in
    // the private array.  A private array indexed by a per-lane depth is scratch memory, and 64 lanes at 64 depths are 64
    // lines per push and per pop - as many as the node fetch itself, out of the same L1 miss bandwidth that bounds the walk.
    __shared__ unsigned s_stack[kLdsStack][64];       // (indexed, not through a pointer: a 64-bit pointer was spilled and reloaded at every push)
    unsigned stack[2 * kStack - kLdsStack];  // BLAS entries sit above the TLAS entries of the same ray
    const size_t deep_base = DEEP ? (size_t)blockIdx.x * s.deep_cap * 64u + lane : 0u;       // one wave per workgroup in the DEEP kernel
    Ray world, ray;                        // `ray` is the active one (object space inside an instance)
    VdHit res;
    [[maybe_unused]] float t_lo = 0.0f;    // RANGE: the lower end of the ray's interval
    unsigned ray_id = 0;
    // ((st & kBusy) != 0u) / ((st & kDone) != 0u) / ((st & kInBlas) != 0u) live as bits of one per-lane word: as `bool`s they are lane masks in scalar registers, and every
    // assignment under divergent control flow is mask algebra (550 of the loop's 1060 instructions were s_and / s_or / s_andn2)
    unsigned st = 0;
    constexpr unsigned kBusy = 1u, kDone = 2u, kInBlas = 4u, kOvf = 8u, kBadLeaf = 16u, kBadEntry = 32u;
    bool exhausted = false;               // wave-uniform
    unsigned head = 0, blas_base = 0;
    unsigned tl_leaf = 0, bvh_index = 0, base_index = 0, vertex_offset = 0;   // tl_leaf: the TLAS leaf node the ray is inside
    uint2 cn = make_uint2(0u, 0u);         // payload of the current node
#ifdef VD_TUNING
    unsigned dbg_outer = 0, dbg_iter = 0, dbg_lanes = 0, dbg_kind[3] = {0, 0, 0}, dbg_ray_steps = 0, dbg_ray_max = 0, dbg_drain = 0, dbg_lone = 0, dbg_few = 0;
    // timeline (words 16..63 of the flag block): [16,17] = earliest wave start (100 MHz ticks), [18..40] = waves that ended in
    // each 0.5 ms slot, [41..63] = stepping iterations done in each slot
    if (lane == 0) atomicMin(reinterpret_cast<unsigned long long*>(overflow + 16), (unsigned long long)wall_clock64());
    unsigned dbg_slot_iter = 0, dbg_slot = 0;
#endif

    auto pop = [&]() {                     // leave the current node
        if (((st & kInBlas) != 0u) && head == blas_base) { st &= ~kInBlas; ray = world; }
        if (head == 0u) { st |= kDone; return; }
        --head;
        unsigned w;
        if (DEEP && head >= 2u * (unsigned)kStack) w = s.deep[deep_base + (size_t)(head - 2u * (unsigned)kStack) * 64u];
        else w = head < (unsigned)kLdsStack ? s_stack[head][lane] : stack[head - (unsigned)kLdsStack];
        if (((st & kInBlas) != 0u)) cn = make_uint2(w & 0x3fffffffu, w >> 30);
        else cn = WIDE ? tl_node_wide(w) : ((w & 0xffffu) ? make_uint2(w, 0xffffffffu) : make_uint2(0u, w >> 16));
    };
    for (;;) {
        // ---- retire finished rays, refill idle lanes ----
        if (((st & kBusy) != 0u) && ((st & kDone) != 0u)) {
#ifdef VD_TUNING
            dbg_ray_max = max(dbg_ray_max, dbg_ray_steps); dbg_ray_steps = 0;
#endif
            if (FAN && (ray_id & 0x80000000u)) {          // a job: its slot takes the result, the ray's minimum is updated
                FanJob* J = src.fan.jobs + (ray_id & 0x7fffffffu);
                if (res.hit) {
                    const unsigned rid = J->ray_id;
                    if (ANY) out_any[rid] = 1u;
                    else {
                        J->lim = res.dist; J->node = tl_instance<WIDE>(s, res.instance); J->tri = res.triangle;
                        atomicMin(src.fan.best + rid, ((unsigned long long)__float_as_uint(res.dist) << 32) | J->key);
                    }
                }
                J->state = (res.hit && !ANY) ? FAN_HIT : FAN_MISS;
            } else
            if (ANY) out_any[ray_id] = res.hit;
            else {
                if (res.hit) res.instance = tl_instance<WIDE>(s, res.instance);      // hits carry the leaf node until here
                if constexpr (RANGE) { if (!res.hit) res.dist = kMaxDist; }          // a miss is the miss record, whatever t_hi was
                out[ray_id] = res;
            }
            st &= ~kBusy;
        }
        const unsigned long long busy_mask = __ballot(((st & kBusy) != 0u));
        if (!exhausted && (unsigned)__popcll(busy_mask) < kRefillBelow) {
            const unsigned long long idle = ~busy_mask;
            const unsigned want = (unsigned)__popcll(idle);
            unsigned base = 0, end = 0, done = 0;                   // single positions from one global counter: the finest balance
            if (lane == 0) base = atomicAdd(src.next, want);
            base = __shfl(base, 0);
            end = base + want;                                      // positions are checked against n_rays below (limit)
            done = end >= n_rays ? 1u : 0u;
            // the position drawn is checked against an explicit upper limit (`pos < limit`), never through a difference: written as
            // `got = base < n_rays ? min(want, n_rays - base) : 0; if (k < got)` the one-wave kernel was compiled WITHOUT the
            // `base < n_rays` guard (v_sub_u32 + v_min_u32, no clamp, no select: profiles/r03_trace_guard_isa.txt) and every
            // draw past the end took `want` rays from beyond the array
            const unsigned limit = n_rays;
            if (!((st & kBusy) != 0u)) {
                const unsigned pos = base + vd_mbcnt(idle);
                if (from_jobs && pos < limit && pos >= base) {
                    const uint4* Jp = reinterpret_cast<const uint4*>(src.fan.jobs + (job_begin + pos));
                    const uint4 j0 = Jp[0], j1 = Jp[1], j2 = Jp[2];
                    const bool skip = j2.z != FAN_PENDING || (ANY && out_any[j1.w] != 0u);      // a filler slot, or the ray is known to be occluded
                    if (skip) { if (j2.z == FAN_PENDING) src.fan.jobs[job_begin + pos].state = FAN_MISS; }
                    else {
                        world.ex = __uint_as_float(j0.x); world.ey = __uint_as_float(j0.y); world.ez = __uint_as_float(j0.z);
                        world.dx = __uint_as_float(j0.w); world.dy = __uint_as_float(j1.x); world.dz = __uint_as_float(j1.y);
                        world.ix = 1.0f / world.dx; world.iy = 1.0f / world.dy; world.iz = 1.0f / world.dz;   // ray_new: inv_dir = 1. / dir
                        ray = world;
                        // only t below the distance found before the fan-out counts - or, when another job of this ray has finished
                        // with a hit meanwhile, t up to and including that distance (an equal t is decided by the keys)
                        float lim = __uint_as_float(j1.z);
                        if (!ANY) {
                            const unsigned bd = (unsigned)(src.fan.best[j1.w] >> 32);
                            if (bd < 0x7f800000u && __uint_as_float(bd + 1u) < lim) lim = __uint_as_float(bd + 1u);      // next float above a positive distance
                        }
                        if constexpr (RANGE) t_lo = fmaxf(rays[j1.w]._pad0, 0.0f);      // no room for it in the job: read again from the ray
                        res.dist = lim; res.hit = 0u; res.instance = 0xffffffffu; res.triangle = 0xffffffffu;
                        const unsigned w = j2.y;                       // the subtree, as the stack held it (pop)
                        cn = WIDE ? tl_node_wide(w) : ((w & 0xffffu) ? make_uint2(w, 0xffffffffu) : make_uint2(0u, w >> 16));
                        ray_id = 0x80000000u | (job_begin + pos); st |= kBusy; st &= ~kDone; st &= ~kInBlas; head = 0; blas_base = 0;
                        if (FAN && kFanAge) s_born[lane] = wave_iters;
                    }
                } else
                if (pos < limit && pos >= base) {
                    const unsigned id = src.order ? src.order[pos] : pos;
                    const float4 a = reinterpret_cast<const float4*>(rays + id)[0], b = reinterpret_cast<const float4*>(rays + id)[1];
                    world.ex = a.x; world.ey = a.y; world.ez = a.z; world.dx = b.x; world.dy = b.y; world.dz = b.z;
                    world.ix = 1.0f / world.dx; world.iy = 1.0f / world.dy; world.iz = 1.0f / world.dz;   // ray_new: inv_dir = 1. / dir
                    ray = world;
                    res.dist = kMaxDist; res.hit = 0u; res.instance = 0xffffffffu; res.triangle = 0xffffffffu;
                    if constexpr (RANGE) { t_lo = fmaxf(a.w, 0.0f); res.dist = fminf(b.w, kMaxDist); }      // VdRay::_pad0, _pad1 of the two loads
                    if constexpr (WIDE) {
                        const VdTlasNodeWide* root = reinterpret_cast<const VdTlasNodeWide*>(s.tlas);
                        cn = make_uint2((root->left | root->right) != 0u ? 1u : 0u, 0u);
                    } else {
                    const VdTlasNode root = s.tlas[0];
                    cn = make_uint2(root.left_right, 0u);          // .y of a TLAS leaf = its node index
                    }
                    ray_id = id; st |= kBusy; st &= ~kDone; st &= ~kInBlas; head = 0; blas_base = 0;
                    if (FAN && kFanAge) s_born[lane] = wave_iters;
                }
            }
            if (done) exhausted = true;     // wave-uniform
        }
        // The supply rule: a wave ends only when its launch's supply is exhausted.  For fresh rays "nobody busy after a draw" can only
        // mean that; for jobs it also happens when every job just drawn was skipped (fillers, finished slots, any-hit rays already
        // known to be occluded) - the wave then goes round once more with nobody stepping and draws again (the counter advances with
        // every draw, so this ends).  Ending there left the positions behind it to the other waves, and when all of them ended so,
        // to nobody: those jobs were never walked and an any-hit ray kept the 0 of its first fan-out (profiles/trace_fan_supply.md).
        // (Written as part of this one condition: a `continue` of its own here cost the fan-out's kernels 9 - 30 spilled VGPRs.)
        if (!__ballot(((st & kBusy) != 0u)) && (exhausted || !(FAN && from_jobs))) {
#ifdef VD_TUNING
            if (!exhausted && lane == 0) atomicAdd(overflow + 3, 1u);      // must stay 0 (vd_debug_trace_fan)
#endif
            break;
        }
        if (FAN && exhausted && src.fan.below != 0u && !fan_off) {
            // nothing left to draw and few rays alive here: every ray that is between instances (its stack holds TLAS entries
            // only) becomes jobs and leaves; rays inside an instance go on and are looked at again when the wave next gets here
            const bool live = (st & kBusy) != 0u;
            if ((unsigned)__popcll(__ballot(live)) < src.fan.below || drain_iters >= kFanGrace) {
                if (drain_iters >= kFanGrace) drain_iters = kFanGrace - kFanAgain;
                const bool can = live && (st & kInBlas) == 0u && (!kFanAge || wave_iters - s_born[kFanAge ? lane : 0u] >= kFanAge);
                // the bottom entry of a ray that came through the reference's root: the true root's second visit (see above)
                unsigned dup_word = 0u;
                if constexpr (WIDE) {      // the root's own record names both children as stack words
                    const VdTlasNodeWide* root = reinterpret_cast<const VdTlasNodeWide*>(s.tlas);
                    if (root->left != 0u && root->left == root->right) {
                        const float4 c0 = s.tpair[0], c1 = s.tpair[1];
                        if (__float_as_uint(c0.w) != 0xffffffffu) dup_word = tl_word_wide(make_uint2(__float_as_uint(c0.w), __float_as_uint(c1.w)));
                    }
                } else {
                    const unsigned lr = s.tlas[0].left_right, l = lr & 0xffffu;
                    if (lr != 0u && l == (lr >> 16)) { const unsigned w2 = s.tlas[l].left_right; dup_word = w2 != 0u ? w2 : (l << 16); }
                }
                const bool dup = can && head != 0u && dup_word != 0u && (ray_id & 0x80000000u) == 0u && s_stack[0][lane] == dup_word;
                const unsigned n_ent = can ? head - (dup ? 1u : 0u) : 0u;
                const unsigned m = can ? n_ent + 2u : 0u;           // the result so far, the node it is at, the stack entries
                unsigned incl = m;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) { const unsigned v = __shfl_up(incl, off); if (lane >= (unsigned)off) incl += v; }
                const unsigned total = __shfl(incl, 63);
                if (total != 0u) {
                    unsigned base = 0;
                    if (lane == 0) base = atomicAdd(src.fan.append, total);
                    base = __shfl(base, 0);
                    if (base + total > src.fan.cap) {
                        // list full: nobody of this wave fans out (now or later); the part of the reservation that lies inside
                        // the list is filled with slots that say "nothing here"
                        for (unsigned k = lane; k < total && base + k < src.fan.cap; k += 64u) src.fan.jobs[base + k].state = FAN_NULL;
                        fan_off = true;
                    } else if (can) {
                        unsigned rid = ray_id, pkey = 0u;
                        if (ray_id & 0x80000000u) {                 // a job fans out again: one more digit behind its own key
                            FanJob* P = src.fan.jobs + (ray_id & 0x7fffffffu);
                            rid = P->ray_id; pkey = P->key;
                            P->state = FAN_MISS;                    // its result so far moves to the new slot below
                        }
                        const unsigned shift = 8u * (3u - src.fan.level);
                        uint4* O = reinterpret_cast<uint4*>(src.fan.jobs + (base + incl - m));
                        const uint4 r0 = make_uint4(__float_as_uint(world.ex), __float_as_uint(world.ey), __float_as_uint(world.ez), __float_as_uint(world.dx));
                        const unsigned dyb = __float_as_uint(world.dy), dzb = __float_as_uint(world.dz), limb = __float_as_uint(res.dist);
                        // digit 0: what the ray has found so far, as a finished job
                        const unsigned inst0 = res.hit ? tl_instance<WIDE>(s, res.instance) : 0xffffffffu;
                        O[0] = r0; O[1] = make_uint4(dyb, dzb, limb, rid);
                        O[2] = make_uint4(pkey, inst0, (res.hit && !ANY) ? FAN_HIT : FAN_MISS, res.triangle);
                        if (res.hit && !ANY) atomicMin(src.fan.best + rid, ((unsigned long long)limb << 32) | pkey);
                        if ((ray_id & 0x80000000u) == 0u) {         // a ray's first fan-out: its record so far (a miss unless a job says otherwise)
                            if (ANY) out_any[rid] = res.hit;
                            else {
                                VdHit h = res; h.instance = inst0;
                                if constexpr (RANGE) { if (!res.hit) h.dist = kMaxDist; }      // limb above stays t_hi: the jobs start from it
                                out[rid] = h;
                            }
                        }
                        // digit 1: the node the ray is at; digits 2..: the stack, top first
                        O[3] = r0; O[4] = make_uint4(dyb, dzb, limb, rid);
                        O[5] = make_uint4(pkey | (1u << shift), WIDE ? tl_word_wide(cn) : (cn.x != 0u ? cn.x : (cn.y << 16)), FAN_PENDING, 0u);
                        for (unsigned e = 0; e < n_ent; ++e) {
                            const unsigned at = head - 1u - e;
                            const unsigned w = at < (unsigned)kLdsStack ? s_stack[at][lane] : stack[at - (unsigned)kLdsStack];
                            O[6u + 3u * e] = r0; O[7u + 3u * e] = make_uint4(dyb, dzb, limb, rid);
                            O[8u + 3u * e] = make_uint4(pkey | ((2u + e) << shift), w, FAN_PENDING, 0u);
                        }
                        st &= ~kBusy;
                    }
                    if (!__ballot(((st & kBusy) != 0u))) break;
                }
            }
        }
        // ---- interior steps (bvh.wgsl:56-74 and 104-121) and instance entries (bvh.wgsl:78-87) ----
        // A TLAS leaf is an instance to enter: instance -> inv_transform + mesh -> MeshInfo -> the mesh's root node -> its two
        // children is a chain of four dependent fetches, taken 140 times per ray on the stress scene (2000 overlapping
        // instances; 1.9 BLAS steps per entry: most entries end at the root's children) against 475 interior steps.  The
        // entry record of the leaf (entry_records_kernel: one 128-byte line per TLAS node, rewritten at every call) holds
        // all of it, so an entry is ONE trip to L2 (and a second read of the same line out of L1) and runs the root's step in
        // the same iteration - same values, same arithmetic.
        // The wave leaves the loop to serve the lanes that wait - at a BLAS leaf, or finished - once `yield` of them do
        // (or nobody steps any more): leaves are rare next to steps (13 against 615 per ray on the stress scene), so waiting
        // for every lane to reach one would idle most of the wave, and serving each at once would run the triangle code
        // for one lane at a time.
        const unsigned n_busy = (unsigned)__popcll(__ballot(((st & kBusy) != 0u)));
#ifdef VD_TUNING
        ++dbg_outer;
#endif
        for (;;) {
            // PREP: a lane at a BLAS leaf steps too - its fetch is one de-indexed triangle (36 contiguous bytes), in flight
            // together with the other lanes' node pairs and entry records: one trip to memory per iteration whatever the
            // lanes are doing.  (Indexed leaves are two dependent fetches of another shape: served outside the loop.)
            const bool leaf = ((st & kInBlas) != 0u) && cn.y != 0u;
            const bool stepping = ((st & kBusy) != 0u) && !((st & kDone) != 0u) && (PREP || !leaf);
            const unsigned n_step = (unsigned)__popcll(__ballot(stepping));
            if (n_step == 0u || n_busy - n_step >= s.yield) break;
            if (FAN && kFanAge) wave_iters = (unsigned)__builtin_amdgcn_readfirstlane((int)(wave_iters + 1u));
            if (FAN && exhausted && src.fan.below != 0u && !fan_off) {      // time to fan out what is still alive?
                drain_iters = (unsigned)__builtin_amdgcn_readfirstlane((int)(drain_iters + 1u));      // (kept in a scalar register: it was a spilled VGPR otherwise)
                if (drain_iters >= kFanGrace) break;
            }
#ifdef VD_TUNING
            ++dbg_iter; dbg_lanes += n_step; if (stepping) ++dbg_ray_steps; if (exhausted) ++dbg_drain;
            if ((dbg_iter & 15u) == 0u) {       // every 16 iterations: which 0.5 ms slot are we in
                const unsigned long long t0 = *reinterpret_cast<volatile unsigned long long*>(overflow + 16);
                const unsigned slot = min(22u, (unsigned)((wall_clock64() - t0) / 200000ull));
                if (slot != dbg_slot) { if (lane == 0 && dbg_slot_iter) atomicAdd(overflow + 41 + dbg_slot, dbg_slot_iter); dbg_slot = slot; dbg_slot_iter = 0; }
                dbg_slot_iter += 16u;
            }
            if (n_busy == 1u) ++dbg_lone; else if (n_busy <= 4u) ++dbg_few;
            dbg_kind[0] += (unsigned)__popcll(__ballot(stepping && leaf)); dbg_kind[1] += (unsigned)__popcll(__ballot(stepping && !leaf && !((st & kInBlas) != 0u) && cn.x == 0u));
            dbg_kind[2] += (unsigned)__popcll(__ballot(stepping && !leaf && !((st & kInBlas) != 0u) && cn.x != 0u));
#endif
            if (!stepping) continue;
            const bool enter = !((st & kInBlas) != 0u) && cn.x == 0u;
            const char* p0; const char* p1;
            unsigned idx0 = 0u, idx1 = 0u;
            if (PREP && leaf) {               // triangle cn.x of the mesh: the vertices fetch_vertex (bvh.wgsl:30-33) returns
                p0 = reinterpret_cast<const char*>(s.tris + 9u * ((size_t)(base_index / 3u) + cn.x));
                p1 = p0 + sizeof(VdBvhNode);
            } else if (enter) {               // the leaf's entry record: matrix rows + mesh id
                p0 = reinterpret_cast<const char*>(s.irec + 4u * (size_t)cn.y);
                p1 = p0 + sizeof(VdBvhNode);
            } else if (((st & kInBlas) != 0u)) {
                p0 = reinterpret_cast<const char*>(s.bvh + (bvh_index + cn.x));
                p1 = p0 + sizeof(VdBvhNode);
            } else if constexpr (WIDE) {      // both children as ONE line: the node's own record
                p0 = reinterpret_cast<const char*>(s.tpair + 4u * (size_t)cn.y);
                p1 = p0 + sizeof(VdBvhNode);
            } else {
                idx0 = cn.x & 0xffffu; idx1 = cn.x >> 16u;       // both children as ONE line: the pair record at the left child's index
                p0 = reinterpret_cast<const char*>(s.tpair + 4u * (size_t)idx0);
                p1 = p0 + sizeof(VdTlasNode);
            }
            // one set of registers for either kind of lane: an entering lane's matrix rows travel with the other lanes' child pairs
            float4 a0 = reinterpret_cast<const float4*>(p0)[0], a1 = reinterpret_cast<const float4*>(p0)[1];
            float4 b0 = reinterpret_cast<const float4*>(p1)[0], b1 = reinterpret_cast<const float4*>(p1)[1];
            bool do_pop = false;              // one pop site for both kinds of lane
            if (PREP && leaf) {               // bvh.wgsl:48-55, one triangle per iteration, in leaf order
                const float v0[3] = {a0.x, a0.y, a0.z}, v1[3] = {a0.w, a1.x, a1.y}, v2[3] = {a1.z, a1.w, b0.x};
                float hit = res.dist;
                if (intersect_trig<RANGE>(ray, v0, v1, v2, hit, t_lo)) {
                    res.dist = hit; res.hit = 1u; res.instance = tl_leaf; res.triangle = cn.x;
                    if (ANY) { st |= kDone; continue; }
                }
                if (--cn.y == 0u) do_pop = true; else ++cn.x;
            } else {
            if (enter) {
                // (inv_transform * vec4(eye, 1.)).xyz and (inv_transform * vec4(dir, 0.)).xyz; a0, a1, b0 = rows 0..2 of the matrix
                tl_leaf = cn.y;
                ray.ex = ((a0.x * world.ex + a0.y * world.ey) + a0.z * world.ez) + a0.w * 1.0f;
                ray.ey = ((a1.x * world.ex + a1.y * world.ey) + a1.z * world.ez) + a1.w * 1.0f;
                ray.ez = ((b0.x * world.ex + b0.y * world.ey) + b0.z * world.ez) + b0.w * 1.0f;
                ray.dx = ((a0.x * world.dx + a0.y * world.dy) + a0.z * world.dz) + a0.w * 0.0f;
                ray.dy = ((a1.x * world.dx + a1.y * world.dy) + a1.z * world.dz) + a1.w * 0.0f;
                ray.dz = ((b0.x * world.dx + b0.y * world.dy) + b0.z * world.dz) + b0.w * 0.0f;
                ray.ix = 1.0f / ray.dx; ray.iy = 1.0f / ray.dy; ray.iz = 1.0f / ray.dz;
                if (__float_as_uint(b1.y) != 0u) { st |= kBadEntry; st |= kDone; continue; }   // the leaf's instance lies outside the buffer
                // the mesh's words and its root's children: the mesh record (a handful of lines that stay in L1)
                const float4* Mr = s.mrec + 8u * (size_t)__float_as_uint(b1.x);
                const float4 idv = Mr[0];
                a0 = Mr[4]; a1 = Mr[5]; b0 = Mr[6]; b1 = Mr[7];
                bvh_index = __float_as_uint(idv.x); base_index = __float_as_uint(idv.y); vertex_offset = __float_as_uint(idv.z);
                const unsigned rw = __float_as_uint(idv.w);            // the mesh's root: left_first | count << 30 (traverse_bvh starts there)
                if (rw == 0xffffffffu) { st |= kBadEntry; st |= kDone; continue; }   // mesh root / its children outside the buffer
                st |= kInBlas;
                blas_base = head;
                cn = make_uint2(rw & 0x3fffffffu, rw >> 30);
                if (cn.y != 0u) continue;                                // a mesh of <= 3 triangles: its root is a leaf
            } else if (WIDE) {
                // a child index outside the array, or an interior node without a left child (records_wide_kernel)
                if (!((st & kInBlas) != 0u) && __float_as_uint(a0.w) == 0xffffffffu) { st |= kBadEntry; st |= kDone; continue; }
            } else if (!((st & kInBlas) != 0u) && __float_as_uint(a1.w) != idx1) {
                // the pair record at idx0 was written for another right child: some unreachable slot of the TLAS array names
                // the same left child (records_kernel) - read the two nodes themselves
                const float4* n0 = reinterpret_cast<const float4*>(s.tlas + idx0);
                const float4* n1 = reinterpret_cast<const float4*>(s.tlas + idx1);
                a0 = n0[0]; a1 = n0[1]; b0 = n1[0]; b1 = n1[1];
            }
            const float mn0[3] = {a0.x, a0.y, a0.z}, mx0[3] = {a1.x, a1.y, a1.z};
            const float mn1[3] = {b0.x, b0.y, b0.z}, mx1[3] = {b1.x, b1.y, b1.z};
            float min_dist = intersect_aabb(ray, mn0, mx0, res.dist);
            float max_dist = intersect_aabb(ray, mn1, mx1, res.dist);
            // payload of a child: BLAS {left_first, count}; TLAS {left_right, its own node index}
            uint2 near = make_uint2(__float_as_uint(a0.w), ((st & kInBlas) != 0u) ? __float_as_uint(a1.w) : idx0);
            uint2 far = make_uint2(__float_as_uint(b0.w), ((st & kInBlas) != 0u) ? __float_as_uint(b1.w) : idx1);
            if constexpr (WIDE) {      // a TLAS record holds its children's cn words where a BLAS node holds {left_first, count}
                near.y = __float_as_uint(a1.w); far.y = __float_as_uint(b1.w);
            }
            if (min_dist > max_dist) {
                const uint2 tu = near; near = far; far = tu;
                const float tf = min_dist; min_dist = max_dist; max_dist = tf;
            }
            if (min_dist >= res.dist) do_pop = true;
            else {
            // far child: the BLAS loop keeps it on `<=` (a missed child, 1e30, is pushed while nothing is hit yet),
            // the TLAS loop on `<`
            const bool blas_now = (st & kInBlas) != 0u;
            if (max_dist < res.dist || (blas_now && max_dist == res.dist)) {
                if (head + 1u > 2u * (unsigned)kStack) {
                    if (!DEEP) {          // out of entries: this ray is walked again by the second pass (its record is rewritten there)
                        if (s.ovf_bits) {
                            const unsigned rid = (FAN && (ray_id & 0x80000000u)) ? src.fan.jobs[ray_id & 0x7fffffffu].ray_id : ray_id;
                            atomicOr(s.ovf_bits + (rid >> 5), 1u << (rid & 31u));
                        }
                        st |= kOvf; st |= kDone; continue;
                    }
                    if (head - 2u * (unsigned)kStack >= s.deep_cap) { st |= kOvf; st |= kDone; continue; }
                }
                if (blas_now && far.y > 3u) st |= kBadLeaf;   // not representable in a stack entry
                const unsigned w_blas = far.x | (far.y << 30), w_tlas = WIDE ? tl_word_wide(far) : (far.x != 0u ? far.x : (far.y << 16));
                const unsigned w = blas_now ? w_blas : w_tlas;
                if (DEEP && head >= 2u * (unsigned)kStack) s.deep[deep_base + (size_t)(head - 2u * (unsigned)kStack) * 64u] = w;
                else if (head < (unsigned)kLdsStack) s_stack[head][lane] = w; else stack[head - (unsigned)kLdsStack] = w;
                ++head;
            }
            cn = near;
            }
            }
            if (do_pop) pop();
        }
        if (PREP || !((st & kBusy) != 0u) || ((st & kDone) != 0u) || !(((st & kInBlas) != 0u) && cn.y != 0u)) continue;     // only lanes at an indexed BLAS leaf go on
        {
            // ---- BLAS leaf (bvh.wgsl:48-55) ----
            for (unsigned k = 0; k < cn.y; ++k) {
                const unsigned idx = cn.x + k;
                float a0[3], a1[3], a2[3];
                if (PREP) {          // the same three vertices fetch_vertex (bvh.wgsl:30-33) returns, stored side by side
                    const float* T = s.tris + 9u * ((size_t)(base_index / 3u) + idx);
                    a0[0] = T[0]; a0[1] = T[1]; a0[2] = T[2]; a1[0] = T[3]; a1[1] = T[4]; a1[2] = T[5]; a2[0] = T[6]; a2[1] = T[7]; a2[2] = T[8];
                } else {
                    const unsigned i0 = vertex_offset + s.indices[base_index + 3u * idx + 0u];
                    const unsigned i1 = vertex_offset + s.indices[base_index + 3u * idx + 1u];
                    const unsigned i2 = vertex_offset + s.indices[base_index + 3u * idx + 2u];
                    const float* v0 = s.verts + 3u * (size_t)i0;
                    const float* v1 = s.verts + 3u * (size_t)i1;
                    const float* v2 = s.verts + 3u * (size_t)i2;
                    a0[0] = v0[0]; a0[1] = v0[1]; a0[2] = v0[2]; a1[0] = v1[0]; a1[1] = v1[1]; a1[2] = v1[2]; a2[0] = v2[0]; a2[1] = v2[1]; a2[2] = v2[2];
                }
                float hit = res.dist;
                if (intersect_trig<RANGE>(ray, a0, a1, a2, hit, t_lo)) {
                    res.dist = hit; res.hit = 1u; res.instance = tl_leaf; res.triangle = idx;
                    if (ANY) break;
                }
            }
            if (ANY && res.hit) st |= kDone; else pop();
        }
    }
#ifdef VD_TUNING
    if (lane == 0) {       // wave totals -> the words after the flag and the ray counter (vd_debug_trace_counters)
        atomicAdd(overflow + 4, dbg_outer); atomicAdd(overflow + 5, dbg_iter);
        atomicAdd(reinterpret_cast<unsigned long long*>(overflow + 6), (unsigned long long)dbg_lanes);
        atomicAdd(overflow + 8, dbg_kind[0]); atomicAdd(overflow + 9, dbg_kind[1]); atomicAdd(overflow + 10, dbg_kind[2]);
        atomicAdd(overflow + 12, dbg_drain);
        atomicMax(overflow + 13, dbg_iter);                 // the wave that iterates longest ...
        atomicMax(overflow + 14, dbg_lone);                 // ... and the longest stretches with one / two to four ((st & kBusy) != 0u) lanes
        atomicMax(overflow + 15, dbg_few);
        if (dbg_slot_iter) atomicAdd(overflow + 41 + dbg_slot, dbg_slot_iter);
        const unsigned long long t0 = *reinterpret_cast<volatile unsigned long long*>(overflow + 16);
        atomicAdd(overflow + 18 + min(22u, (unsigned)((wall_clock64() - t0) / 200000ull)), 1u);
    }
    atomicMax(overflow + 11, dbg_ray_max);
#endif
    if (st & kOvf) atomicOr(overflow, 1u);
    if (st & kBadLeaf) atomicOr(overflow, 2u);
    if (st & kBadEntry) atomicOr(overflow, 4u);
}

// Entry points: one wave per workgroup, the persistent grid = 24 waves per CU.  The first pass takes the scene's buffers
// as plain kernel arguments (SceneArgs) and the ray count by value; the deep second pass takes the Scene struct and its list.
struct SceneArgs { const VdTlasNode* tlas; const VdInstance* inst; const VdMeshInfo* meshes; const VdBvhNode* bvh;
                   const float* verts; const unsigned* indices; unsigned n_meshes, yield; const float4* irec; const float4* tpair; const float4* mrec;
                   unsigned* ovf_bits; };
constexpr int kFanWps = 5;
template <bool ANY, bool FAN>      // FAN: the fan-out's code is compiled in (calls that run as one launch use the kernel without it)
__global__ __launch_bounds__(64, FAN ? kFanWps : 6)      // second argument (HIP): waves per SIMD = 24 per CU; the fan-out's kernels take 96 registers at 5 per SIMD
                                                         // instead of spilling 9-12 at 6 (124 -> 129 / 192 -> 202 Mrays/s, profiles/r04_ab_trace_fan_wps.log)
void trace_single_kernel(SceneArgs a, const VdRay* __restrict__ rays, unsigned n_rays, VdHit* __restrict__ out, unsigned* __restrict__ out_any,
                         unsigned* __restrict__ overflow, unsigned* next_ray, const unsigned* __restrict__ gate, Fan fan) {
    if (gate && *gate == 0u) return;          // the call de-indexed the leaves itself and that went well: the other kernel runs
    const Scene s{a.tlas, a.inst, a.meshes, a.bvh, a.verts, a.indices, a.n_meshes, nullptr, a.irec, a.tpair, a.mrec, a.yield, a.ovf_bits};
    const RaySource src{nullptr, n_rays, next_ray, fan};
    trace_body<ANY, false, FAN>(s, rays, src, out, out_any, overflow);
}
template <bool ANY, bool FAN>
__global__ __launch_bounds__(64, FAN ? kFanWps : 6)
void trace_single_prep_kernel(SceneArgs a, const VdRay* __restrict__ rays, unsigned n_rays, VdHit* __restrict__ out, unsigned* __restrict__ out_any,
                              unsigned* __restrict__ overflow, unsigned* next_ray, const float* __restrict__ tris,
                              const unsigned* __restrict__ gate, Fan fan) {
    if (gate && *gate != 0u) return;          // the call's own de-indexing met an index range it cannot use: the indexed kernel runs
    const Scene s{a.tlas, a.inst, a.meshes, a.bvh, a.verts, a.indices, a.n_meshes, tris, a.irec, a.tpair, a.mrec, a.yield, a.ovf_bits};
    const RaySource src{nullptr, n_rays, next_ray, fan};
    trace_body<ANY, true, FAN>(s, rays, src, out, out_any, overflow);
}
// The second pass: the rays listed in `list` (their ids, *n_list of them), one wave per workgroup, the stack beyond 128
// entries in s.deep.  Rare by construction - a handful of rays of a deep scene - so it is one plain launch.
template <bool ANY, bool PREP>
__global__ __launch_bounds__(64, 4)
void trace_deep_kernel(Scene s, const VdRay* __restrict__ rays, const unsigned* __restrict__ list, const unsigned* __restrict__ n_list,
                       VdHit* __restrict__ out, unsigned* __restrict__ out_any, unsigned* __restrict__ overflow, unsigned* next_ray) {
    const unsigned n = *n_list;
    const RaySource src{list, n, next_ray};
    trace_body<ANY, PREP, false, true>(s, rays, src, out, out_any, overflow);
}
// The same three entry points over a wide top level (vd_trace_wide*): a.tlas / s.tlas point at VdTlasNodeWide, irec and tpair at
// the one record table (records_wide_kernel).
template <bool ANY, bool PREP, bool FAN>
__global__ __launch_bounds__(64, FAN ? kFanWps : 6)
void trace_wide_kernel(SceneArgs a, const VdRay* __restrict__ rays, unsigned n_rays, VdHit* __restrict__ out, unsigned* __restrict__ out_any,
                       unsigned* __restrict__ overflow, unsigned* next_ray, const float* __restrict__ tris, const unsigned* __restrict__ gate, Fan fan) {
    if (gate && (*gate != 0u) == PREP) return;          // as above: the de-indexing of this call decides which of the two kernels walks
    const Scene s{a.tlas, a.inst, a.meshes, a.bvh, a.verts, a.indices, a.n_meshes, PREP ? tris : nullptr, a.irec, a.tpair, a.mrec, a.yield, a.ovf_bits};
    const RaySource src{nullptr, n_rays, next_ray, fan};
    trace_body<ANY, PREP, FAN, false, true>(s, rays, src, out, out_any, overflow);
}
template <bool ANY, bool PREP>
__global__ __launch_bounds__(64, 4)
void trace_deep_wide_kernel(Scene s, const VdRay* __restrict__ rays, const unsigned* __restrict__ list, const unsigned* __restrict__ n_list,
                            VdHit* __restrict__ out, unsigned* __restrict__ out_any, unsigned* __restrict__ overflow, unsigned* next_ray) {
    const unsigned n = *n_list;
    const RaySource src{list, n, next_ray};
    trace_body<ANY, PREP, false, true, true>(s, rays, src, out, out_any, overflow);
}
// VD_OPT_TRACE_RAY_RANGE: the same five kernels with RANGE as one more template parameter - overloads by the length of the
// template parameter list, so the kernels above keep their symbols as well as their code (tests/test_trace_wide_abi.py finds
// them by symbol) and the inventory of tests/test_isa_protocols.py, which goes by name, sees no new kernel.  Same arguments.  Only
// RANGE = true is ever instantiated (launch_first_pass, trace_deep_pass).
// Launch bounds: t_lo is one more VGPR that lives through the stepping loop, and four narrow instantiations cannot hold their
// sibling's bound with it (1 - 4 dwords spilled and reloaded in the loop): they get one wave per SIMD less, as the fan-out's kernels
// did (kFanWps) - 5 (96 registers) for the closest-hit kernels without the fan-out's code, 4 (128) for the two with it that spilled
// at 5.  Every other RANGE instantiation fits its sibling's bound and keeps it.  No RANGE instantiation spills a VGPR
// (profiles/trace_ray_range.md has the table).
constexpr int range_wps(bool any, bool prep, bool fan) {
    if (!fan) return any ? 6 : 5;                                      // trace_single_kernel<0, 0>, trace_single_prep_kernel<0, 0>
    return ((!any && !prep) || (any && prep)) ? kFanWps - 1 : kFanWps;     // trace_single_kernel<0, 1>, trace_single_prep_kernel<1, 1>
}
template <bool ANY, bool FAN, bool RANGE>
__global__ __launch_bounds__(64, range_wps(ANY, false, FAN))
void trace_single_kernel(SceneArgs a, const VdRay* __restrict__ rays, unsigned n_rays, VdHit* __restrict__ out, unsigned* __restrict__ out_any,
                         unsigned* __restrict__ overflow, unsigned* next_ray, const unsigned* __restrict__ gate, Fan fan) {
    if (gate && *gate == 0u) return;
    const Scene s{a.tlas, a.inst, a.meshes, a.bvh, a.verts, a.indices, a.n_meshes, nullptr, a.irec, a.tpair, a.mrec, a.yield, a.ovf_bits};
    const RaySource src{nullptr, n_rays, next_ray, fan};
    trace_body<ANY, false, FAN, false, false, RANGE>(s, rays, src, out, out_any, overflow);
}
template <bool ANY, bool FAN, bool RANGE>
__global__ __launch_bounds__(64, range_wps(ANY, true, FAN))
void trace_single_prep_kernel(SceneArgs a, const VdRay* __restrict__ rays, unsigned n_rays, VdHit* __restrict__ out, unsigned* __restrict__ out_any,
                              unsigned* __restrict__ overflow, unsigned* next_ray, const float* __restrict__ tris,
                              const unsigned* __restrict__ gate, Fan fan) {
    if (gate && *gate != 0u) return;
    const Scene s{a.tlas, a.inst, a.meshes, a.bvh, a.verts, a.indices, a.n_meshes, tris, a.irec, a.tpair, a.mrec, a.yield, a.ovf_bits};
    const RaySource src{nullptr, n_rays, next_ray, fan};
    trace_body<ANY, true, FAN, false, false, RANGE>(s, rays, src, out, out_any, overflow);
}
template <bool ANY, bool PREP, bool RANGE>
__global__ __launch_bounds__(64, 4)
void trace_deep_kernel(Scene s, const VdRay* __restrict__ rays, const unsigned* __restrict__ list, const unsigned* __restrict__ n_list,
                       VdHit* __restrict__ out, unsigned* __restrict__ out_any, unsigned* __restrict__ overflow, unsigned* next_ray) {
    const unsigned n = *n_list;
    const RaySource src{list, n, next_ray};
    trace_body<ANY, PREP, false, true, false, RANGE>(s, rays, src, out, out_any, overflow);
}
template <bool ANY, bool PREP, bool FAN, bool RANGE>
__global__ __launch_bounds__(64, FAN ? kFanWps : 6)
void trace_wide_kernel(SceneArgs a, const VdRay* __restrict__ rays, unsigned n_rays, VdHit* __restrict__ out, unsigned* __restrict__ out_any,
                       unsigned* __restrict__ overflow, unsigned* next_ray, const float* __restrict__ tris, const unsigned* __restrict__ gate, Fan fan) {
    if (gate && (*gate != 0u) == PREP) return;
    const Scene s{a.tlas, a.inst, a.meshes, a.bvh, a.verts, a.indices, a.n_meshes, PREP ? tris : nullptr, a.irec, a.tpair, a.mrec, a.yield, a.ovf_bits};
    const RaySource src{nullptr, n_rays, next_ray, fan};
    trace_body<ANY, PREP, FAN, false, true, RANGE>(s, rays, src, out, out_any, overflow);
}
template <bool ANY, bool PREP, bool RANGE>
__global__ __launch_bounds__(64, 4)
void trace_deep_wide_kernel(Scene s, const VdRay* __restrict__ rays, const unsigned* __restrict__ list, const unsigned* __restrict__ n_list,
                            VdHit* __restrict__ out, unsigned* __restrict__ out_any, unsigned* __restrict__ overflow, unsigned* next_ray) {
    const unsigned n = *n_list;
    const RaySource src{list, n, next_ray};
    trace_body<ANY, PREP, false, true, true, RANGE>(s, rays, src, out, out_any, overflow);
}
// bitmap of the first pass -> list of ray ids (any order: a ray's record depends on the ray alone).  n_words = ceil(n_rays / 32);
// bits of the last word that name no ray of this call are dropped: the list holds n_rays ids, rays[] and out[] n_rays records.
__global__ __launch_bounds__(256) void ovf_list_kernel(const unsigned* __restrict__ bits, unsigned n_words, unsigned n_rays, unsigned* __restrict__ list,
                                                       unsigned* __restrict__ count) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_words) return;
    unsigned w = bits[i];
    if (n_rays - i * 32u < 32u) w &= (1u << (n_rays - i * 32u)) - 1u;      // i < n_words: at least one ray in this word
    if (w == 0u) return;
    unsigned at = atomicAdd(count, (unsigned)__popc(w));
    while (w) { const unsigned b = (unsigned)__builtin_ctz(w); list[at++] = i * 32u + b; w &= w - 1u; }
}

// fan-out, between two launches: the jobs appended so far are the next launch's supply
__global__ void fan_snapshot_kernel(const unsigned* append, unsigned cap, unsigned* end) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *end = min(*append, cap);
}
// fan-out, after the last launch: of a ray's finished jobs the one holding the minimum {distance, key} writes the ray's record
__global__ __launch_bounds__(256) void fan_resolve_kernel(const FanJob* __restrict__ jobs, const unsigned* __restrict__ append, unsigned cap,
                                                          const unsigned long long* __restrict__ best, VdHit* __restrict__ out) {
    const unsigned n = min(*append, cap);
    for (unsigned j = blockIdx.x * 256u + threadIdx.x; j < n; j += gridDim.x * 256u) {
        const FanJob J = jobs[j];
        if (J.state != FAN_HIT) continue;
        if (best[J.ray_id] != (((unsigned long long)__float_as_uint(J.lim) << 32) | J.key)) continue;
        VdHit h; h.dist = J.lim; h.hit = 1u; h.instance = J.node; h.triangle = J.tri;
        out[J.ray_id] = h;
    }
}

// Shadow rays of the reference's deferred pass (src/bin/raytraced_shadows.wgsl:97): origin = pos + nor * 0.0001,
// dir = light.position - pos (not normalised: t is in units of the light vector, and the pass ignores it).
__global__ __launch_bounds__(256) void shadow_rays_kernel(const float* __restrict__ pos, const float* __restrict__ nor, unsigned n,
                                                          float lx, float ly, float lz, float t_min, float t_max, VdRay* __restrict__ rays) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float px = pos[3u * i], py = pos[3u * i + 1u], pz = pos[3u * i + 2u];
    VdRay r;
    r.eye[0] = px + nor[3u * i] * 0.0001f; r.eye[1] = py + nor[3u * i + 1u] * 0.0001f; r.eye[2] = pz + nor[3u * i + 2u] * 0.0001f;
    r._pad0 = t_min;
    r.dir[0] = lx - px; r.dir[1] = ly - py; r.dir[2] = lz - pz;
    r._pad1 = t_max;
    rays[i] = r;
}

// One ray per pixel as the CPU harness makes them (src/bin/bvh_cpu.rs:71-83): pixel i -> x = (i % W) / W,
// y = (i / H) / H (the source divides by HEIGHT for the row; W == H == 640 there), ((x, y) - 0.5) * (2, -2),
// eye = (clip_to_world * (x, y, 1, 1)).xyz / .w, dir = normalize((clip_to_world * (x, y, 0, 1)).xyz).
struct Mat4 { float m[16]; };
__global__ __launch_bounds__(256) void primary_rays_kernel(Mat4 c2w, unsigned width, unsigned height, unsigned n, float t_min, float t_max,
                                                                  VdRay* __restrict__ rays) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float* M = c2w.m;
    float x = (float)(i % width) / (float)width;
    float y = (float)(i / height) / (float)height;
    x = (x - 0.5f) * 2.0f;
    y = (y - 0.5f) * -2.0f;
    float p[4], t[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        p[r] = ((M[r] * x + M[4 + r] * y) + M[8 + r] * 1.0f) + M[12 + r] * 1.0f;
        t[r] = ((M[r] * x + M[4 + r] * y) + M[8 + r] * 0.0f) + M[12 + r] * 1.0f;
    }
    const float rl = 1.0f / sqrtf((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
    VdRay r;
    r.eye[0] = p[0] / p[3]; r.eye[1] = p[1] / p[3]; r.eye[2] = p[2] / p[3]; r._pad0 = t_min;
    r.dir[0] = t[0] * rl; r.dir[1] = t[1] * rl; r.dir[2] = t[2] * rl; r._pad1 = t_max;
    rays[i] = r;
}

// `Bvh::traverse_iter` of the CPU harness (crates/bvh/src/blas.rs:247-295): one mesh, no TLAS.  It is NOT the WGSL
// walk above: the slab test divides by dir (intersection.rs:47-55), the triangle test is two-sided with EPS = 1e-4
// on the determinant and on t (intersection.rs:68-92), a child whose box is missed is never pushed, the near child
// is pushed first (so the far one is popped first), and pruning uses the closest hit so far or 1e30.  One lane per
// ray walks exactly that sequence.  The reference's stack holds 32 entries and panics past them (blas.rs:298-324);
// here 128, and overflow is an error code.  out_dist[r] = closest t, or -1 for Dist::Miss.
constexpr int kIterStack = 128;
struct DistRs { bool hit; float t; };
__device__ __forceinline__ DistRs intersect_aabb_rs(float ox, float oy, float oz, float dx, float dy, float dz,
                                                    const float* mn, const float* mx, float t) {
    const float ax = (mn[0] - ox) / dx, ay = (mn[1] - oy) / dy, az = (mn[2] - oz) / dz;
    const float bx = (mx[0] - ox) / dx, by = (mx[1] - oy) / dy, bz = (mx[2] - oz) / dz;
    const float tmax = min3(fmaxf(ax, bx), fmaxf(ay, by), fmaxf(az, bz));
    const float tmin = max3(fminf(ax, bx), fminf(ay, by), fminf(az, bz));
    return DistRs{tmax >= tmin && tmin < t && tmax > 0.0f, tmin};
}
// intersection.rs:68-92; t, or -1 for Miss
__device__ __forceinline__ float ray_intersect_rs(float ox, float oy, float oz, float dx, float dy, float dz,
                                                  const float* v0, const float* v1, const float* v2) {
    constexpr float EPS = 0.0001f;
    const float e1x = v1[0] - v0[0], e1y = v1[1] - v0[1], e1z = v1[2] - v0[2];
    const float e2x = v2[0] - v0[0], e2y = v2[1] - v0[1], e2z = v2[2] - v0[2];
    const float hx = dy * e2z - e2y * dz, hy = dz * e2x - e2z * dx, hz = dx * e2y - e2x * dy;   // dir x edge2
    const float a = dot3(e1x, e1y, e1z, hx, hy, hz);
    if (-EPS < a && a < EPS) return -1.0f;
    const float f = 1.0f / a;
    const float sx = ox - v0[0], sy = oy - v0[1], sz = oz - v0[2];
    const float u = f * dot3(sx, sy, sz, hx, hy, hz);
    if (!(0.0f <= u && u <= 1.0f)) return -1.0f;
    const float qx = sy * e1z - e1y * sz, qy = sz * e1x - e1z * sx, qz = sx * e1y - e1x * sy;   // s x edge1
    const float v = f * dot3(dx, dy, dz, qx, qy, qz);
    if (v < 0.0f || u + v > 1.0f) return -1.0f;
    const float t = f * dot3(e2x, e2y, e2z, qx, qy, qz);
    return t > EPS ? t : -1.0f;
}

__global__ __launch_bounds__(64) void traverse_iter_kernel(const VdBvhNode* __restrict__ nodes, const float* __restrict__ verts,
                                                           const unsigned* __restrict__ indices, const VdRay* __restrict__ rays,
                                                           unsigned n_rays, float* __restrict__ out_dist, unsigned* __restrict__ overflow) {
    const unsigned r = blockIdx.x * 64u + threadIdx.x;
    if (r >= n_rays) return;
    const float4 e4 = reinterpret_cast<const float4*>(rays + r)[0], d4 = reinterpret_cast<const float4*>(rays + r)[1];
    const float ox = e4.x, oy = e4.y, oz = e4.z, dx = d4.x, dy = d4.y, dz = d4.z;
    unsigned stack[kIterStack];
    int head = 0;
    stack[head++] = 0u;
    float hit = -1.0f;   // Dist::Miss
    bool ovf = false;
    while (head > 0) {
        const VdBvhNode node = nodes[stack[--head]];
        if (node.count > 0u) {
            for (unsigned i = 0; i < node.count; ++i) {
                const unsigned* idx = indices + 3u * (size_t)(node.left_first + i);
                const float d = ray_intersect_rs(ox, oy, oz, dx, dy, dz, verts + 3u * (size_t)idx[0], verts + 3u * (size_t)idx[1],
                                                 verts + 3u * (size_t)idx[2]);
                if (d >= 0.0f) hit = hit >= 0.0f ? fminf(hit, d) : d;
            }
        } else {
            unsigned min_index = node.left_first, max_index = node.left_first + 1u;
            const VdBvhNode mc = nodes[min_index], xc = nodes[max_index];
            const float lim = hit >= 0.0f ? hit : kMaxDist;
            DistRs min_dist = intersect_aabb_rs(ox, oy, oz, dx, dy, dz, mc.min, mc.max, lim);
            DistRs max_dist = intersect_aabb_rs(ox, oy, oz, dx, dy, dz, xc.min, xc.max, lim);
            // derive(PartialOrd) on enum Dist { Hit(f32), Miss } (intersection.rs:22-26): Hit(x) < Miss
            const bool gt = min_dist.hit != max_dist.hit ? !min_dist.hit : (min_dist.hit && min_dist.t > max_dist.t);
            if (gt) {
                const unsigned ti = min_index; min_index = max_index; max_index = ti;
                const DistRs td = min_dist; min_dist = max_dist; max_dist = td;
            }
            if (!min_dist.hit) continue;
            if (head + 2 > kIterStack) { ovf = true; break; }
            stack[head++] = min_index;
            if (max_dist.hit) stack[head++] = max_index;
        }
    }
    out_dist[r] = hit;
    if (ovf) atomicOr(overflow, 1u);
}

// `Bvh::traverse` (crates/bvh/src/blas.rs:211-245), the RECURSIVE walk of the reference (its only call
// site is commented out at src/bin/bvh_cpu.rs:86).  traverse(node, t): Miss when the node's box is missed under t
// (same slab test as traverse_iter, intersection.rs:47-55); a leaf folds its triangles into t (`t = t.min(dist)`); an
// interior node calls left THEN right - no near / far ordering - each with the t found so far; every entered node
// returns Hit(t).  The returned t is only ever the running minimum handed on, so the recursion equals a pre-order walk
// with one running t and a stack of pending right children; one lane per ray runs that.  Quirk kept: a ray that enters
// the root box and hits nothing returns Hit(t0) - the t it was GIVEN - and Miss (-1) only when the root box is missed.
__global__ __launch_bounds__(64) void traverse_rec_kernel(const VdBvhNode* __restrict__ nodes, const float* __restrict__ verts,
                                                          const unsigned* __restrict__ indices, const VdRay* __restrict__ rays,
                                                          unsigned n_rays, float t0, float* __restrict__ out_dist,
                                                          unsigned* __restrict__ overflow) {
    const unsigned r = blockIdx.x * 64u + threadIdx.x;
    if (r >= n_rays) return;
    const float4 e4 = reinterpret_cast<const float4*>(rays + r)[0], d4 = reinterpret_cast<const float4*>(rays + r)[1];
    const float ox = e4.x, oy = e4.y, oz = e4.z, dx = d4.x, dy = d4.y, dz = d4.z;
    unsigned stack[kIterStack];
    int head = 0;
    float t = t0;
    bool ovf = false, entered_root = false;
    unsigned cur = 0u;
    bool have = true;
    while (have) {
        const VdBvhNode node = nodes[cur];
        have = false;
        const DistRs box = intersect_aabb_rs(ox, oy, oz, dx, dy, dz, node.min, node.max, t);   // blas.rs:220-222
        if (box.hit) {
            if (cur == 0u) entered_root = true;
            if (node.count > 0u) {                                                             // blas.rs:223-235
                for (unsigned i = 0; i < node.count; ++i) {
                    const unsigned* idx = indices + 3u * (size_t)(node.left_first + i);
                    const float d = ray_intersect_rs(ox, oy, oz, dx, dy, dz, verts + 3u * (size_t)idx[0], verts + 3u * (size_t)idx[1],
                                                     verts + 3u * (size_t)idx[2]);
                    if (d >= 0.0f) t = fminf(t, d);
                }
            } else {                                                                           // blas.rs:236-243: left, then right
                if (head + 1 > kIterStack) { ovf = true; break; }
                stack[head++] = node.left_first + 1u;
                cur = node.left_first; have = true;
                continue;
            }
        }
        if (head > 0) { cur = stack[--head]; have = true; }
    }
    out_dist[r] = entered_root ? t : -1.0f;                                                    // blas.rs:244 / :221
    if (ovf) atomicOr(overflow, 1u);
}

// Per-call records: what the walk reads at a TLAS step and when it enters an instance, re-laid so that each is ONE line.
// The bound of this kernel family is the number of distinct lines a CU can fetch (tools/probe_gather.hip:
// profiles/r03_probe_gather.log), so the lines per ray are what counts:
//   tpair[idx0]  (64 B) the two children of a TLAS node - tlas[idx0], tlas[idx1] - side by side at the LEFT child's index
//                (a TLAS step used to fetch two nodes at unrelated indices = two lines).  The left copy's unused
//                instance_idx word holds idx1 as a tag: a slot written for another right child (an unreachable slot of
//                the array naming the same left child) is detected and the step reads the two nodes themselves.  When
//                several slots name one left child, exactly ONE writes the record - the lowest node index
//                (pair_owner_kernel: atomicMin into an owner word, then records_kernel writes only as the owner) - so a
//                record is never a mixture of two writers' stores;
//   irec[k]      (64 B) for a TLAS leaf k: rows 0..2 of its instance's inv_transform (row r = {M[r], M[4 + r], M[8 + r],
//                M[12 + r]}: the operands of (inv_transform * vec4(p, w)).r in source order), {mesh id, bad-instance flag};
//   mrec[m]      (128 B) per mesh: {bvh_index, base_index, vertex_offset, root.left_first | root.count << 30} and the 64
//                bytes of the root's two children: `instance_intersect` (bvh.wgsl:78-87) + the first step of `traverse_bvh`
//                (bvh.wgsl:35-76) used to be instance -> MeshInfo -> root -> children, four dependent fetches, 140 times
//                per ray on the stress scene; few meshes, so these lines stay in L1.
// Written at the start of EVERY trace call from the scene's own buffers (<= 65 536 nodes: a few microseconds), so
// instances, TLAS nodes and meshes may change between calls as before.  A mesh whose root or root children lie outside
// the buffers gets 0xffffffff as its root word: a ray that ENTERS it reports VD_ERR_INVALID_ARG.
constexpr unsigned kTlasSlots = 65536;              // 16-bit child indices (bvh.wgsl:105-106)
__global__ __launch_bounds__(256) void pair_owner_kernel(const VdTlasNode* __restrict__ tlas, unsigned n_nodes, unsigned* __restrict__ owner) {
    const unsigned k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n_nodes) return;
    const unsigned lr = tlas[k].left_right;
    if (lr != 0u && (lr & 0xffffu) < n_nodes && (lr >> 16u) < n_nodes) atomicMin(owner + (lr & 0xffffu), k);
}

// (the two records every top level shares, as functions for records_wide_kernel; records_kernel below keeps its own text:
//  written through these it compiled to other instructions)
__device__ __forceinline__ void mesh_record(const VdMeshInfo* __restrict__ meshes, const VdBvhNode* __restrict__ bvh, unsigned n_bvh,
                                            float4* __restrict__ mrec, unsigned k) {
    {
        const VdMeshInfo mesh = meshes[k];
        float4* R = mrec + 8u * (size_t)k;
        unsigned rw = 0xffffffffu;
        if (mesh.bvh_index < n_bvh) {
            const VdBvhNode root = bvh[mesh.bvh_index];
            if (root.count <= 3u && root.left_first < (1u << 30)) {        // else: not a BvhBuilder tree (blas.rs:108)
                if (root.count != 0u) rw = root.left_first | (root.count << 30);
                else {
                    const size_t c = (size_t)mesh.bvh_index + root.left_first;
                    if (c + 1u < n_bvh) {
                        const float4* src = reinterpret_cast<const float4*>(bvh + c);
                        R[4] = src[0]; R[5] = src[1]; R[6] = src[2]; R[7] = src[3];
                        rw = root.left_first;
                    }
                }
            }
        }
        R[0] = make_float4(__uint_as_float(mesh.bvh_index), __uint_as_float(mesh.base_index), __uint_as_float((unsigned)mesh.vertex_offset),
                           __uint_as_float(rw));
    }
}
__device__ __forceinline__ void entry_record(const VdInstance* __restrict__ inst, unsigned n_inst, unsigned n_meshes, unsigned instance_idx,
                                             float4* __restrict__ R) {
    if (instance_idx >= n_inst) { R[3] = make_float4(0.0f, __uint_as_float(1u), 0.0f, 0.0f); return; }
    const VdInstance* I = inst + instance_idx;
    const float* M = I->inv_transform;
    R[0] = make_float4(M[0], M[4], M[8], M[12]);
    R[1] = make_float4(M[1], M[5], M[9], M[13]);
    R[2] = make_float4(M[2], M[6], M[10], M[14]);
    R[3] = make_float4(__uint_as_float(min(I->mesh, n_meshes - 1u)), __uint_as_float(0u), 0.0f, 0.0f);
}
__global__ __launch_bounds__(256) void records_kernel(const VdTlasNode* __restrict__ tlas, unsigned n_nodes, const VdInstance* __restrict__ inst,
                                                      unsigned n_inst, const VdMeshInfo* __restrict__ meshes, unsigned n_meshes,
                                                      const VdBvhNode* __restrict__ bvh, unsigned n_bvh, float4* __restrict__ irec,
                                                      float4* __restrict__ tpair, float4* __restrict__ mrec, const unsigned* __restrict__ owner) {
    const unsigned k = blockIdx.x * 256u + threadIdx.x;
    if (k < n_meshes) {
        const VdMeshInfo mesh = meshes[k];
        float4* R = mrec + 8u * (size_t)k;
        unsigned rw = 0xffffffffu;
        if (mesh.bvh_index < n_bvh) {
            const VdBvhNode root = bvh[mesh.bvh_index];
            if (root.count <= 3u && root.left_first < (1u << 30)) {        // else: not a BvhBuilder tree (blas.rs:108)
                if (root.count != 0u) rw = root.left_first | (root.count << 30);
                else {
                    const size_t c = (size_t)mesh.bvh_index + root.left_first;
                    if (c + 1u < n_bvh) {
                        const float4* src = reinterpret_cast<const float4*>(bvh + c);
                        R[4] = src[0]; R[5] = src[1]; R[6] = src[2]; R[7] = src[3];
                        rw = root.left_first;
                    }
                }
            }
        }
        R[0] = make_float4(__uint_as_float(mesh.bvh_index), __uint_as_float(mesh.base_index), __uint_as_float((unsigned)mesh.vertex_offset),
                           __uint_as_float(rw));
    }
    if (k >= n_nodes) return;
    const VdTlasNode node = tlas[k];
    if (node.left_right != 0u) {
        const unsigned idx0 = node.left_right & 0xffffu, idx1 = node.left_right >> 16u;
        if (idx0 < n_nodes && idx1 < n_nodes && owner[idx0] == k) {
            const float4* c0 = reinterpret_cast<const float4*>(tlas + idx0);
            const float4* c1 = reinterpret_cast<const float4*>(tlas + idx1);
            float4 lo = c0[1]; lo.w = __uint_as_float(idx1);
            float4* P = tpair + 4u * (size_t)idx0;
            P[0] = c0[0]; P[1] = lo; P[2] = c1[0]; P[3] = c1[1];
        }
        return;
    }
    float4* R = irec + 4u * (size_t)k;
    if (node.instance_idx >= n_inst) { R[3] = make_float4(0.0f, __uint_as_float(1u), 0.0f, 0.0f); return; }
    const VdInstance* I = inst + node.instance_idx;
    const float* M = I->inv_transform;
    R[0] = make_float4(M[0], M[4], M[8], M[12]);
    R[1] = make_float4(M[1], M[5], M[9], M[13]);
    R[2] = make_float4(M[2], M[6], M[10], M[14]);
    R[3] = make_float4(__uint_as_float(min(I->mesh, n_meshes - 1u)), __uint_as_float(0u), 0.0f, 0.0f);
}

// The records of a WIDE top level: ONE 64-byte record per node, at the node's own index (grid-stride: up to 2^25 + 1 nodes).
//   leaf (left == right == 0): its entry record, as above;
//   interior: {min0, x0 | max0, y0 | min1, x1 | max1, y1} - the boxes of both children with the words the walk holds for
//   a node it is at: x = 1 interior / 0 leaf, y = the child's index (tl_node).  x0 = 0xffffffff marks a node no ray may
//   step: a child index outside the array, or left == 0 (what a leaf's word would say).
// Every slot below n_nodes is written by its own node and no child index above n_nodes is ever followed, so nothing is
// filled beforehand and no record has two writers - what the narrow walk needs owners and tags for.
__global__ __launch_bounds__(256) void records_wide_kernel(const VdTlasNodeWide* __restrict__ tlas, unsigned n_nodes, const VdInstance* __restrict__ inst,
                                                           unsigned n_inst, const VdMeshInfo* __restrict__ meshes, unsigned n_meshes,
                                                           const VdBvhNode* __restrict__ bvh, unsigned n_bvh, float4* __restrict__ rec,
                                                           float4* __restrict__ mrec) {
    for (unsigned k = blockIdx.x * 256u + threadIdx.x; k < max(n_nodes, n_meshes); k += gridDim.x * 256u) {
        if (k < n_meshes) mesh_record(meshes, bvh, n_bvh, mrec, k);
        if (k >= n_nodes) continue;
        const uint4* N = reinterpret_cast<const uint4*>(tlas + k);
        const unsigned left = N[0].w, right = N[1].w;
        float4* R = rec + 4u * (size_t)k;
        if (left == 0u && right == 0u) { entry_record(inst, n_inst, n_meshes, N[2].x, R); continue; }
        if (left == 0u || left >= n_nodes || right >= n_nodes) { R[0] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0xffffffffu)); continue; }
        const float4* c0 = reinterpret_cast<const float4*>(tlas + left);
        const float4* c1 = reinterpret_cast<const float4*>(tlas + right);
        float4 a0 = c0[0], a1 = c0[1], b0 = c1[0], b1 = c1[1];
        a0.w = __uint_as_float((__float_as_uint(a0.w) | __float_as_uint(a1.w)) != 0u ? 1u : 0u); a1.w = __uint_as_float(left);
        b0.w = __uint_as_float((__float_as_uint(b0.w) | __float_as_uint(b1.w)) != 0u ? 1u : 0u); b1.w = __uint_as_float(right);
        R[0] = a0; R[1] = a1; R[2] = b0; R[3] = b1;
    }
}

// De-indexed leaf triangles: tris[9 * (base_index / 3 + t)] = the three vertices fetch_vertex (bvh.wgsl:30-33) returns for
// triangle t of the mesh, i.e. vertices[vertex_offset + indices[base_index + 3 t + c]].
__global__ __launch_bounds__(256) void prepare_tris_kernel(const VdMeshInfo* __restrict__ meshes, const float* __restrict__ verts,
                                                           const unsigned* __restrict__ indices, unsigned n_indices, unsigned n_vertices,
                                                           float* __restrict__ tris, unsigned* __restrict__ err) {
    const VdMeshInfo m = meshes[blockIdx.y];
    const unsigned n_tri = m.index_count / 3u;
    if (m.base_index % 3u != 0u || (size_t)m.base_index + m.index_count > n_indices) { if (threadIdx.x == 0 && blockIdx.x == 0) atomicOr(err, 4u); return; }
    for (unsigned t = blockIdx.x * 256u + threadIdx.x; t < n_tri; t += gridDim.x * 256u) {
        float* T = tris + 9u * ((size_t)(m.base_index / 3u) + t);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const unsigned vi = (unsigned)m.vertex_offset + indices[m.base_index + 3u * t + c];
            if (vi >= n_vertices) { atomicOr(err, 4u); T[3 * c] = T[3 * c + 1] = T[3 * c + 2] = 0.0f; continue; }
            T[3 * c] = verts[3u * (size_t)vi]; T[3 * c + 1] = verts[3u * (size_t)vi + 1u]; T[3 * c + 2] = verts[3u * (size_t)vi + 2u];
        }
    }
}

// ---- VD_OPT_TRACE_TIGHT_TLAS: a private top level over TIGHT world boxes ------------------------------------------
// The reference seeds every TLAS leaf box with the OBJECT-space mesh box (tlas.rs:39: the fold starts from
// [mesh.min, mesh.max]), so all leaves overlap around the origin and a ray enters most instances near it (145 of 2000 on
// the stress scene).  Which instances a ray ENTERS does not change what it hits: inside an instance only the root's
// children and below are tested (bvh.wgsl:35-76), all within the mesh's root box.  The private top level therefore
// bounds each instance by the eight corners of its BLAS ROOT box under `transform` - no seed - padded by 2e-5 of the
// box's largest coordinate (the rounding of transforming the ray in versus the corners out is ~1e-6 of that) PLUS how far
// `inv_transform`, which is all the walk uses, puts the geometry from where `transform` puts the corners (per axis, from
// T * Tinv - I: see the kernel), and clusters those boxes with the same agglomerative builder.  Used only where it is provably the same geometry: the
// instance's inv_transform must invert its transform (|T * Tinv - I| <= 1e-3 per element) and every corner must be
// finite.  ONE instance that fails either makes vd_trace_prepare_dev decline the option for the whole scene (it keeps
// the scene's own top level; VdTraceAccelInfo.tight_fallback_instances says how many failed): the hits of an instance
// whose inverse is stale lie outside its box, so whether the reference finds them depends on its visit order, and a
// top level with non-finite boxes may have dropped clusters (tlas.rs:87-105 finds no partner for a NaN area) that only
// the reference's own build reproduces.

// One instance's tight box, or false (mn / mx then hold nothing): the rule above, for both node types.
__device__ __forceinline__ bool tight_box(const VdInstance* __restrict__ inst, unsigned i, const VdMeshInfo* __restrict__ meshes, unsigned n_meshes,
                                          const VdBvhNode* __restrict__ bvh, unsigned n_bvh, float (&mn)[3], float (&mx)[3]) {
    const float* T = inst[i].transform;
    const float* V = inst[i].inv_transform;
    const VdMeshInfo m = meshes[min(inst[i].mesh, n_meshes - 1u)];
    bool ok = m.bvh_index < n_bvh;
    float worst = 0.0f;
    float E[3][4];                             // rows 0..2 of T * Tinv - I: where the walk's geometry sits relative to T's
    for (int r = 0; r < 4 && ok; ++r)
        for (int c = 0; c < 4; ++c) {
            float a = 0.0f;
            for (int k = 0; k < 4; ++k) a += T[4 * k + r] * V[4 * c + k];        // (T * Tinv)[r][c], column-major storage
            const float e = fabsf(a - (r == c ? 1.0f : 0.0f));
            if (r < 3) E[r][c] = e;
            worst = fmaxf(worst, e);
        }
    ok = ok && worst <= 1e-3f;                 // false for NaN too
    for (int k = 0; k < 3; ++k) { mn[k] = 3e38f; mx[k] = -3e38f; }
    float dev[3] = {0.0f, 0.0f, 0.0f};
    if (ok) {
        const VdBvhNode root = bvh[m.bvh_index];
        const float b[2][3] = {{root.min[0], root.min[1], root.min[2]}, {root.max[0], root.max[1], root.max[2]}};
        for (int c = 0; c < 8; ++c) {
            const float px = b[c & 1][0], py = b[(c >> 1) & 1][1], pz = b[(c >> 2) & 1][2];
            float w[3];
            for (int k = 0; k < 3; ++k) {
                w[k] = ((T[k] * px + T[4 + k] * py) + T[8 + k] * pz) + T[12 + k];
                ok = ok && fabsf(w[k]) < 1e30f;       // finite and inside the format's own range (MAX_DIST)
                mn[k] = fminf(mn[k], w[k]); mx[k] = fmaxf(mx[k], w[k]);
            }
            // The walk takes rays into the instance with inv_transform ALONE, so the geometry it sees is Tinv^-1 * p, not
            // T * p: with T * Tinv = I + E that is (I + E)^-1 * (T p) = T p - E (T p) + O(E^2) - off by at most
            // sum_c |E[k][c]| |(T p)_c| + |E[k][3]| along axis k (a float inverse of an instance 2 000 units out leaves
            // E ~ 1e-4 in the translation column; one nudged by 5e-4 without its inverse passes the 1e-3 test too).
            for (int k = 0; k < 3; ++k) dev[k] = fmaxf(dev[k], ((E[k][0] * fabsf(w[0]) + E[k][1] * fabsf(w[1])) + E[k][2] * fabsf(w[2])) + E[k][3]);
        }
    }
    if (ok) {
        float big = 0.0f;
        for (int k = 0; k < 3; ++k) big = fmaxf(big, fmaxf(fabsf(mn[k]), fabsf(mx[k])));
        for (int k = 0; k < 3; ++k) {
            const float pad = (2e-5f * big + 1e-30f) + 1.01f * dev[k];        // rounding of ray-in versus corners-out + the inverse's own error
            mn[k] -= pad; mx[k] += pad;
        }
    }
    return ok;
}
// A scene's own leaf of instance i sits at i + 1 in every top level a vd_tlas_* builder of the narrow layout made: an instance
// that does not qualify keeps that box.  A WIDE scene's leaves may sit anywhere (voidin_abi.h), so there - and wherever node
// i + 1 is not that leaf - the box is everything; it is never walked (one such instance makes the accel decline).
template <typename Node>
__global__ __launch_bounds__(256) void tight_boxes_kernel(const VdInstance* __restrict__ inst, unsigned n_inst, const VdMeshInfo* __restrict__ meshes,
                                                          unsigned n_meshes, const VdBvhNode* __restrict__ bvh, unsigned n_bvh,
                                                          const Node* __restrict__ scene_tlas, unsigned n_scene_nodes,
                                                          float* __restrict__ boxes, unsigned* __restrict__ n_fallback) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_inst) return;
    float mn[3], mx[3];
    if (!tight_box(inst, i, meshes, n_meshes, bvh, n_bvh, mn, mx)) {
        atomicAdd(n_fallback, 1u);
        bool own_leaf = false;
        if constexpr (std::is_same<Node, VdTlasNode>::value)
            own_leaf = i + 1u < n_scene_nodes && scene_tlas[i + 1u].left_right == 0u && scene_tlas[i + 1u].instance_idx == i;
        for (int k = 0; k < 3; ++k) {
            mn[k] = own_leaf ? scene_tlas[i + 1u].min[k] : -1e30f;
            mx[k] = own_leaf ? scene_tlas[i + 1u].max[k] : 1e30f;
        }
    }
    for (int k = 0; k < 3; ++k) { boxes[6u * i + k] = mn[k]; boxes[6u * i + 3 + k] = mx[k]; }
}

// The reference's build ends with one merge too many (tlas.rs:59 `while node_indices > 0`): node 2n has the true root
// 2n - 1 as BOTH children and node 0 is its copy, so a ray that misses everything walks the tree twice.  The private
// top level starts at the true root.
__global__ void tight_root_kernel(VdTlasNode* nodes, unsigned n) {
    if (threadIdx.x == 0 && blockIdx.x == 0 && n >= 2u) nodes[0] = nodes[2u * n - 1u];
}

// ---- the private top level as an LBVH (VD_OPT_TRACE_TIGHT_TLAS = 2): the builder of vd_tlas_build_lbvh* (tlas.hip:
// vd_tlas_lbvh_from_boxes) over the tight boxes, on all CUs in ~0.1 ms, so it can follow moving instances every frame
// (vd_trace_accel_update_dev); the agglomerative builder (= 1) makes the better tree and takes the reference's
// sequential chain to do it.  Node 0 is the true root there and node 2n is nobody's child: the walk sees 2n nodes.

// WIDE: the scene's top level is VdTlasNodeWide (vd_trace_wide*).  Same call, except that the records are one table of
// n_tlas_nodes x 64 B that needs no fill (records_wide_kernel), in an arena of its own (ctx->trace_wide) so that the narrow
// calls' scratch does not grow with a wide scene's node count, and the wide instantiations of the kernels walk.
template <bool WIDE> using SceneOf = std::conditional_t<WIDE, VdTraceSceneWide, VdTraceScene>;

// What one trace call will do, decided before anything is launched (as pass1_plan does in cull.hip).  The call's arena:
// [256 B flags and counters][TLAS child pairs, 64 B x 65 536][entry records, 64 B x 65 536][pair owners][mesh records][de-indexed triangles][fan-out]
// (pairs and entry records for all 65 536 indices a 16-bit child field can name: a stray index reads a poisoned slot, not
// beyond; WIDE: one table of 64 B per node and no owners), the fan-out as [256 B control words][best: 8 B per ray][jobs: 48 B x cap].
struct TracePlan {
    size_t pair_bytes, irec_bytes, owner_bytes, tris_at, tris_bytes, fan_at, best_bytes, total;
    bool auto_prep;                        // the call de-indexes the leaves itself, into [tris_at, tris_at + tris_bytes)
    unsigned waves, phases, fan_cap;       // the persistent grid, launches of the call (1: no fan-out), job slots
    unsigned yield, ovf_words;             // Scene::yield; words of the overflow bitmap
    bool range;                            // VD_OPT_TRACE_RAY_RANGE: the RANGE instantiations walk (read at every call)
};
template <bool WIDE>
TracePlan trace_plan(VdCtx* ctx, const SceneOf<WIDE>* sc, bool prepared, uint32_t n_rays) {
    TracePlan p;
    p.pair_bytes = (size_t)64 * (WIDE ? sc->n_tlas_nodes : kTlasSlots);
    p.irec_bytes = WIDE ? 0 : (size_t)64 * kTlasSlots;
    p.owner_bytes = WIDE ? 0 : (size_t)4 * kTlasSlots;
    const size_t mrec_bytes = (size_t)128 * sc->n_meshes;
    p.tris_at = 256 + p.pair_bytes + p.irec_bytes + p.owner_bytes + ((mrec_bytes + 255) & ~(size_t)255);
    // A call that was not given prepared leaves de-indexes them itself when that is cheap next to the walk (one pass over the
    // index buffer, 36 B per triangle into the scratch: 5 us for the stress scene's 131 k triangles, 20 us for the harness
    // scene's 1.2 M) - the plain vd_trace_dev then walks at the prepared rate.  Not for few rays over a big scene,
    // not with more meshes than one launch's gridDim.y, and only up to 2 Mi triangles
    // (72 MB of the context's grow-only scratch, kept for its lifetime); VD_OPT_TRACE_AUTO_PREPARE = 2 raises that to
    // 16 Mi (576 MB), 0 turns it off.  vd_trace_prepare_dev is the explicit form without a limit.
    const size_t n_tri = sc->n_indices / 3u;
    const long long auto_opt = ctx->option(VD_OPT_TRACE_AUTO_PREPARE, 1);
    p.auto_prep = !prepared && auto_opt != 0 && n_tri > 0 && sc->n_vertices > 0 && sc->n_meshes <= 65535u &&
                  n_tri <= ((size_t)1 << (auto_opt >= 2 ? 24 : 21)) && (size_t)n_rays * 8u >= n_tri;
    p.tris_bytes = p.auto_prep ? (((size_t)36 * n_tri + 64 + 255) & ~(size_t)255) : 0;
    p.fan_at = p.tris_at + p.tris_bytes;
    // fan-out (kFan*): calls with at least one ray per lane of the grid, scenes with enough instances for a ray to be long.
    p.waves = (unsigned)ctx->num_cus * (unsigned)std::min<long long>(kWavesPerCu, std::max<long long>(1, ctx->option(VD_OPT_TRACE_WAVES, kWavesPerCu)));
    p.phases = (unsigned)std::min<long long>(4, std::max<long long>(1, ctx->option(VD_OPT_TRACE_FAN, kFanPhases)));
    if ((size_t)n_rays < (size_t)p.waves * 64u || sc->n_instances < 64u) p.phases = 1u;
    // The fan-out's kernels cost ~15 % where no ray lives long enough to fan out (more code, spilled registers, launches that find
    // nothing to do): a call remembers how many jobs it made (trace_flags), and while the last call over the same top level made fewer
    // than one per 64 rays the next 15 calls over it run as one launch with the plain kernels; then the fan-out is tried again.
    const bool fan_default = ctx->option(VD_OPT_TRACE_FAN, -1) < 0;
    if (p.phases > 1u && fan_default && ctx->fan_rest(sc->tlas_nodes, sc->n_tlas_nodes, sc->n_instances)) p.phases = 1u;
    p.fan_cap = (unsigned)std::min<size_t>((size_t)1 << 21, (size_t)n_rays * 2u);
    if (ctx->option(VD_OPT_TRACE_FAN_SLOTS, -1) >= 0) p.fan_cap = (unsigned)std::min<long long>(p.fan_cap, ctx->option(VD_OPT_TRACE_FAN_SLOTS, -1));      // tests: a list that fills up
    p.best_bytes = ((size_t)n_rays * 8u + 255) & ~(size_t)255;
    p.total = p.fan_at + (p.phases > 1u ? 256 + p.best_bytes + (size_t)p.fan_cap * sizeof(FanJob) : 0);
    p.yield = (unsigned)std::max<long long>(1, ctx->option(VD_OPT_TRACE_YIELD, kYieldDefault));
    p.ovf_words = (n_rays + 31u) / 32u;
    p.range = ctx->option(VD_OPT_TRACE_RAY_RANGE, 0) == 1;
    return p;
}
// the fan-out's part of the arena (nothing behind these pointers when plan.phases == 1)
struct FanMem { unsigned* ctl; unsigned long long* best; FanJob* jobs; };      // ctl: [0] append, [p] supply counter of launch p >= 1, [8 + p] end of launch p's supply (it begins at [8 + p - 1])
FanMem fan_mem(const TracePlan& p, char* arena) {
    char* const at = arena + p.fan_at;
    return {reinterpret_cast<unsigned*>(at), reinterpret_cast<unsigned long long*>(at + 256), reinterpret_cast<FanJob*>(at + 256 + p.best_bytes)};
}

// The overflow bitmap, one bit per ray: "ran out of its 128 stack entries" (trace_deep_pass).  All zero between calls: zeroed
// when (re)allocated and again after a call that set any (or left early), so a call that overflows nowhere pays nothing for
// it.  A call marks it dirty here and clean (ctx->trace_ovf_dirty = false) when it has ended with every bit zero again.
int ovf_acquire(VdCtx* ctx, unsigned ovf_words, unsigned** d_ovf) {
    const size_t before = ctx->trace_ovf_bytes;      // the size, not the pointer: a grown buffer may come back at the address just freed
    const int rc = vd_ensure(ctx, &ctx->trace_ovf, &ctx->trace_ovf_bytes, (size_t)ovf_words * 4u + 4u);
    if (rc) return rc;
    if (ctx->trace_ovf_bytes != before || ctx->trace_ovf_dirty) VD_HIP_CHECK(ctx, hipMemsetAsync(ctx->trace_ovf, 0, ctx->trace_ovf_bytes, ctx->stream));
    ctx->trace_ovf_dirty = true;       // until this call has ended cleanly
    *d_ovf = reinterpret_cast<unsigned*>(ctx->trace_ovf);
    return VD_OK;
}

// The per-call records of the scene, behind the arena's first 256 bytes.  Narrow: every slot poisoned, then the pair owners,
// then pairs, entry records and mesh records.  WIDE: one table - a node is a leaf or an interior node - that needs no fill.
struct TraceTables { float4* pair; float4* rec; float4* mrec; };
template <bool WIDE>
int launch_records(VdCtx* ctx, const SceneOf<WIDE>* sc, const TracePlan& p, char* arena, TraceTables* t) {
    t->pair = reinterpret_cast<float4*>(arena + 256);
    t->rec = WIDE ? t->pair : reinterpret_cast<float4*>(arena + 256 + p.pair_bytes);
    unsigned* d_owner = reinterpret_cast<unsigned*>(arena + 256 + p.pair_bytes + p.irec_bytes);
    t->mrec = reinterpret_cast<float4*>(arena + 256 + p.pair_bytes + p.irec_bytes + p.owner_bytes);
    if constexpr (WIDE) {
        const unsigned items = std::max(sc->n_tlas_nodes, sc->n_meshes);
        hipLaunchKernelGGL(records_wide_kernel, dim3(vd_blocks(ctx, items, 256u, 64u)), dim3(256), 0, ctx->stream, sc->tlas_nodes, sc->n_tlas_nodes,
                           sc->instances, sc->n_instances, sc->meshes, sc->n_meshes, sc->bvh_nodes, sc->n_bvh_nodes, t->pair, t->mrec);
    } else {
        VD_HIP_CHECK(ctx, hipMemsetAsync(t->pair, 0xff, p.pair_bytes + p.irec_bytes + p.owner_bytes, ctx->stream));      // no pair slot carries a tag or has an owner yet, every entry record says "bad"
        const unsigned n_rec = std::min(sc->n_tlas_nodes, kTlasSlots);      // nodes past 65 535 cannot be named by a 16-bit child field
        hipLaunchKernelGGL(pair_owner_kernel, dim3((n_rec + 255u) / 256u), dim3(256), 0, ctx->stream, sc->tlas_nodes, n_rec, d_owner);
        hipLaunchKernelGGL(records_kernel, dim3((std::max(n_rec, sc->n_meshes) + 255u) / 256u), dim3(256), 0, ctx->stream, sc->tlas_nodes,
                           n_rec, sc->instances, sc->n_instances, sc->meshes, sc->n_meshes, sc->bvh_nodes, sc->n_bvh_nodes, t->rec, t->pair, t->mrec, d_owner);
    }
    return VD_OK;
}

// The first pass takes the scene as plain kernel arguments: the Scene the host built, field by field (the kernels put it
// together again, with the triangles their own argument).
SceneArgs scene_args(const Scene& s) {
    return {s.tlas, s.inst, s.meshes, s.bvh, s.verts, s.indices, s.n_meshes, s.yield, s.irec, s.tpair, s.mrec, s.ovf_bits};
}
// two run-time booleans -> the template arguments of a launch: f(std::integral_constant<bool, a>{}, std::integral_constant<bool, b>{})
template <typename F> void with_bools(bool x, bool y, F&& f) {
    using T = std::integral_constant<bool, true>; using N = std::integral_constant<bool, false>;
    if (x) { if (y) f(T{}, T{}); else f(T{}, N{}); }
    else { if (y) f(N{}, T{}); else f(N{}, N{}); }
}

// ... and a third one, behind the two: g(a, b, std::integral_constant<bool, z>{})
template <typename G> void with_bools(bool x, bool y, bool z, G&& g) {
    with_bools(x, y, [&](auto a, auto b) {
        if (z) g(a, b, std::integral_constant<bool, true>{}); else g(a, b, std::integral_constant<bool, false>{});
    });
}

// What a walk reads and writes besides the scene; flag: the arena's first words - [0] 1 = some ray overflowed, 2 / 4 = refusals, [1] the ray counter, [2] the gate
struct TraceIo { const VdRay* rays; uint32_t n_rays; VdHit* out; uint32_t* any; unsigned* flag; };

// The first pass.  fan-out: launch 0 hands out the rays; launch p >= 1 the jobs appended before it started (fan_snapshot_kernel);
// every launch but the last may append; fan_resolve_kernel writes the records of the rays that were fanned out.
// gate (s.tris de-indexed by this call): non-zero = some mesh's index range cannot be de-indexed - the indexed kernel takes the call.
template <bool WIDE>
void launch_first_pass(VdCtx* ctx, const TracePlan& p, const Scene& s, const unsigned* gate, const TraceIo& io, const FanMem& fm) {
    const SceneArgs a = scene_args(s);
    const float* d_tris = s.tris;
    for (unsigned ph = 0; ph < p.phases; ++ph) {
        Fan fan = {};
        if (p.phases > 1u) {
            fan.jobs = fm.jobs; fan.append = fm.ctl; fan.cap = p.fan_cap; fan.best = fm.best; fan.level = ph;
            fan.below = ph + 1u < p.phases ? kFanBelow : 0u;
            if (ph) { fan.begin = fm.ctl + 8 + (ph - 1); fan.end = fm.ctl + 8 + ph; }
        }
        if (ph) hipLaunchKernelGGL(fan_snapshot_kernel, dim3(1), dim3(64), 0, ctx->stream, fm.ctl, p.fan_cap, fm.ctl + 8 + ph);
        unsigned* next = ph == 0 ? io.flag + 1 : fm.ctl + ph;
        with_bools(io.any != nullptr, p.phases > 1u, p.range, [&](auto any, auto fanned, auto ranged) {
            constexpr bool A = decltype(any)::value, F = decltype(fanned)::value, R = decltype(ranged)::value;
            if constexpr (WIDE) {
                const auto wide_prep = R ? &trace_wide_kernel<A, true, F, true> : &trace_wide_kernel<A, true, F>;
                const auto wide_indexed = R ? &trace_wide_kernel<A, false, F, true> : &trace_wide_kernel<A, false, F>;
                if (d_tris) hipLaunchKernelGGL(wide_prep, dim3(p.waves), dim3(64), 0, ctx->stream, a, io.rays, io.n_rays, io.out, io.any, io.flag,
                                               next, d_tris, gate, fan);
                if (!d_tris || gate) hipLaunchKernelGGL(wide_indexed, dim3(p.waves), dim3(64), 0, ctx->stream, a, io.rays, io.n_rays, io.out, io.any,
                                                        io.flag, next, d_tris, gate, fan);
                return;
            }
            const auto prep = R ? &trace_single_prep_kernel<A, F, true> : &trace_single_prep_kernel<A, F>;
            const auto indexed = R ? &trace_single_kernel<A, F, true> : &trace_single_kernel<A, F>;
            if (d_tris) hipLaunchKernelGGL(prep, dim3(p.waves), dim3(64), 0, ctx->stream, a, io.rays, io.n_rays, io.out, io.any, io.flag,
                                           next, d_tris, gate, fan);
            if (!d_tris || gate) hipLaunchKernelGGL(indexed, dim3(p.waves), dim3(64), 0, ctx->stream, a, io.rays, io.n_rays, io.out, io.any,
                                                    io.flag, next, gate, fan);
        });
    }
    if (p.phases > 1u && !io.any)
        hipLaunchKernelGGL(fan_resolve_kernel, dim3((unsigned)ctx->num_cus * 4u), dim3(256), 0, ctx->stream, fm.jobs, fm.ctl, p.fan_cap, fm.best, io.out);
}

// After the first pass: the flag word, the jobs the fan-out made and the gate come back into host_pinned[0..2] (blocks), the
// context remembers what the fan-out found, and a scene the walk could not make sense of is refused.
template <bool WIDE>
int trace_flags(VdCtx* ctx, const TracePlan& p, const SceneOf<WIDE>* sc, const TraceIo& io, const FanMem& fm) {
    VD_HIP_CHECK(ctx, hipGetLastError());
    VD_HIP_CHECK(ctx, hipMemcpyAsync(ctx->host_pinned, io.flag, 4, hipMemcpyDeviceToHost, ctx->stream));
    if (p.phases > 1u) VD_HIP_CHECK(ctx, hipMemcpyAsync(ctx->host_pinned + 1, fm.ctl, 4, hipMemcpyDeviceToHost, ctx->stream));
    VD_HIP_CHECK(ctx, hipMemcpyAsync(ctx->host_pinned + 2, io.flag + 2, 4, hipMemcpyDeviceToHost, ctx->stream));      // the gate: which of the two kernels walked
    VD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (p.phases > 1u) ctx->fan_remember(sc->tlas_nodes, sc->n_tlas_nodes, sc->n_instances, ctx->host_pinned[1] < io.n_rays / 64u);
    if (ctx->host_pinned[0] & 4u) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_trace: a TLAS leaf's instance, its mesh's root or the root's children lie outside the scene's buffers");
    if (ctx->host_pinned[0] & 2u) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_trace: BVH leaf with more than 3 triangles (BvhBuilder never makes one: blas.rs:108)");
    return VD_OK;
}

// The second pass.  Some rays needed more than the 128 entries a lane holds (the reference's own 24-entry stack is unchecked,
// shaders/utils/stack.wgsl:1-20: it has no answer there at all).  They are walked again, from their start, with the entries
// beyond 128 in a slab of global memory - same visits, same arithmetic, so the records are the ones an unbounded stack gives
// (tests/test_gpu_trace_deep.py holds them against the oracle through the first four sizes).  Entries per lane grow 1 Ki -> 4 Ki -> ...
// until nothing overflows; the slab is waves x 64 lanes x entries x 4 B under a 256 MB budget (fewer waves as it deepens),
// and a stack cannot hold more entries than the scene has nodes (node_bound).
// The largest cap that can run is 4 Mi entries per lane: cap goes 1 Ki, 4 Ki, ..., 1 Mi, 4 Mi, 16 Mi, a wave's part of the slab is
// cap x 256 B, and the limit of 2 GiB per wave passes 4 Mi (1 GiB, by then one wave: the budget only ever lowers the wave
// count to 1) and stops 16 Mi (4 GiB) - 8 Mi, where the limit itself lies, is not a step.  A ray that overflows 128 + 4 Mi
// entries is therefore what the message below says.
template <bool WIDE>
int trace_deep_pass(VdCtx* ctx, const TracePlan& p, const Scene& s, bool prep_walked, size_t node_bound, const TraceIo& io) {
    const size_t list_bytes = ((size_t)io.n_rays * 4u + 255) & ~(size_t)255;
    const size_t budget = (size_t)256 << 20;
    for (size_t cap = 1024;; cap *= 4) {
        const size_t per_wave = cap * 64u * 4u;
        if (per_wave > ((size_t)2 << 30)) VD_FAIL(ctx, VD_ERR_STACK_OVERFLOW, "vd_trace: a ray's traversal stack needs more than 128 + 4 Mi entries");
        const unsigned waves_d = (unsigned)std::max<size_t>(1, std::min<size_t>(p.waves, budget / per_wave));
        const int rc = vd_ensure(ctx, &ctx->trace_deep, &ctx->trace_deep_bytes, 256 + list_bytes + (size_t)waves_d * per_wave);
        if (rc) return rc;
        unsigned* ctl = reinterpret_cast<unsigned*>(ctx->trace_deep);                 // [0] listed rays, [1] supply counter
        unsigned* list = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(ctl) + 256);
        VD_HIP_CHECK(ctx, hipMemsetAsync(ctl, 0, 256, ctx->stream));
        VD_HIP_CHECK(ctx, hipMemsetAsync(io.flag, 0, 4, ctx->stream));
        hipLaunchKernelGGL(ovf_list_kernel, dim3((p.ovf_words + 255u) / 256u), dim3(256), 0, ctx->stream, s.ovf_bits, p.ovf_words, io.n_rays, list, ctl);
        Scene sd = s;
        sd.ovf_bits = nullptr;
        sd.deep = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(list) + list_bytes);
        sd.deep_cap = (unsigned)cap;
        with_bools(io.any != nullptr, prep_walked, p.range, [&](auto any, auto prep, auto ranged) {
            constexpr bool A = decltype(any)::value, P = decltype(prep)::value, R = decltype(ranged)::value;
            const auto deep_wide = R ? &trace_deep_wide_kernel<A, P, true> : &trace_deep_wide_kernel<A, P>;
            const auto deep = R ? &trace_deep_kernel<A, P, true> : &trace_deep_kernel<A, P>;
            if constexpr (WIDE) hipLaunchKernelGGL(deep_wide, dim3(waves_d), dim3(64), 0, ctx->stream, sd, io.rays, list, ctl, io.out,
                                                   io.any, io.flag, ctl + 1);
            else hipLaunchKernelGGL(deep, dim3(waves_d), dim3(64), 0, ctx->stream, sd, io.rays, list, ctl, io.out, io.any, io.flag, ctl + 1);
        });
        vd_time_end(ctx);                                                              // vd_last_gpu_ms covers the second pass too
        VD_HIP_CHECK(ctx, hipGetLastError());
        VD_HIP_CHECK(ctx, hipMemcpyAsync(ctx->host_pinned, io.flag, 4, hipMemcpyDeviceToHost, ctx->stream));
        VD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->host_pinned[0] & 6u) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_trace: the scene's buffers are inconsistent (bad leaf or entry met by the second pass)");
        if (!(ctx->host_pinned[0] & 1u)) break;
        if (cap >= node_bound) VD_FAIL(ctx, VD_ERR_STACK_OVERFLOW, "vd_trace: traversal stack deeper than the scene has nodes (cyclic node arrays?)");
    }
    VD_HIP_CHECK(ctx, hipMemsetAsync(s.ovf_bits, 0, (size_t)p.ovf_words * 4u, ctx->stream));      // all zero between calls (ovf_acquire)
    return VD_OK;
}

// One trace call: plan, arena and bitmap, the flag words, the records, the leaves when the call de-indexes them itself, the
// first pass, its flags, and the second pass for the rays that overflowed.  Blocks.
template <bool WIDE = false>
int launch_trace(VdCtx* ctx, const SceneOf<WIDE>* sc, const float* d_tris, const VdRay* d_rays, uint32_t n_rays, VdHit* d_out, uint32_t* d_any = nullptr) {
    // idle waves keep drawing from the ray counter after the last ray: leave it room below 2^32
    if (n_rays > 0xf0000000u) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_trace: more than 0xf0000000 rays in one call");
    const TracePlan p = trace_plan<WIDE>(ctx, sc, d_tris != nullptr, n_rays);
    int rc = vd_ensure(ctx, WIDE ? &ctx->trace_wide : &ctx->scratch, WIDE ? &ctx->trace_wide_bytes : &ctx->scratch_bytes, p.total);
    if (rc) return rc;
    char* const arena = reinterpret_cast<char*>(WIDE ? ctx->trace_wide : ctx->scratch);
    unsigned* d_ovf = nullptr;
    if ((rc = ovf_acquire(ctx, p.ovf_words, &d_ovf))) return rc;
    vd_time_begin(ctx);
    const TraceIo io{d_rays, n_rays, d_out, d_any, reinterpret_cast<unsigned*>(arena)};
#ifdef VD_TUNING
    VD_HIP_CHECK(ctx, hipMemsetAsync(io.flag, 0, 256, ctx->stream));
    VD_HIP_CHECK(ctx, hipMemsetAsync(io.flag + 16, 0xff, 8, ctx->stream));
#else
    VD_HIP_CHECK(ctx, hipMemsetAsync(io.flag, 0, 64, ctx->stream));
#endif
    const FanMem fm = fan_mem(p, arena);
#ifdef VD_TUNING
    ctx->dbg_fan_wide = WIDE; ctx->dbg_fan_at = p.fan_at;      // vd_debug_trace_fan: where this call's words lie
    ctx->dbg_fan_phases = p.phases; ctx->dbg_fan_waves = p.waves; ctx->dbg_fan_cap = p.fan_cap;
#endif
    if (p.phases > 1u) {
        VD_HIP_CHECK(ctx, hipMemsetAsync(fm.ctl, 0, 256, ctx->stream));
        if (!d_any) VD_HIP_CHECK(ctx, hipMemsetAsync(fm.best, 0xff, p.best_bytes, ctx->stream));
    }
    TraceTables t;
    if ((rc = launch_records<WIDE>(ctx, sc, p, arena, &t))) return rc;
    const unsigned* gate = nullptr;
    if (p.auto_prep) {
        float* tris = reinterpret_cast<float*>(arena + p.tris_at);
        hipLaunchKernelGGL(prepare_tris_kernel, dim3(256, sc->n_meshes), dim3(256), 0, ctx->stream, sc->meshes, sc->vertices, sc->indices, sc->n_indices,
                           sc->n_vertices, tris, io.flag + 2);
        d_tris = tris; gate = io.flag + 2;
    }
    const VdTlasNode* tlas_arg = reinterpret_cast<const VdTlasNode*>(sc->tlas_nodes);      // WIDE: the kernels cast it back (tl_instance)
    const Scene s{tlas_arg, sc->instances, sc->meshes, sc->bvh_nodes, sc->vertices, sc->indices, sc->n_meshes, d_tris, t.rec, t.pair, t.mrec, p.yield, d_ovf};
    launch_first_pass<WIDE>(ctx, p, s, gate, io, fm);
    vd_time_end(ctx);
    if ((rc = trace_flags<WIDE>(ctx, p, sc, io, fm))) return rc;
    if (ctx->host_pinned[0] & 1u) {      // some rays ran out of their 128 entries
        const bool prep_walked = d_tris && (!gate || ctx->host_pinned[2] == 0u);
        rc = trace_deep_pass<WIDE>(ctx, p, s, prep_walked, (size_t)sc->n_tlas_nodes + (size_t)sc->n_bvh_nodes + 2u, io);
        if (rc) return rc;
    }
    ctx->trace_ovf_dirty = false;      // every bit is zero again
    return VD_OK;
}

// the accel's copy of the scene, as the type its `wide` says
template <bool WIDE> SceneOf<WIDE>& accel_scene(VdTraceAccel* a) { if constexpr (WIDE) return a->wscene; else return a->scene; }
template <bool WIDE> const SceneOf<WIDE>& accel_scene(const VdTraceAccel* a) { if constexpr (WIDE) return a->wscene; else return a->scene; }

// New tight boxes from the scene's instances as they are now into a->boxes, the fallback count zeroed before them.
template <bool WIDE>
int launch_tight_boxes(VdCtx* ctx, VdTraceAccel* a, unsigned** d_fb) {
    using Node = std::conditional_t<WIDE, VdTlasNodeWide, VdTlasNode>;
    const SceneOf<WIDE>& sc = accel_scene<WIDE>(a);
    const unsigned n = sc.n_instances;
    *d_fb = reinterpret_cast<unsigned*>(a->boxes + 6 * (size_t)n);
    VD_HIP_CHECK(ctx, hipMemsetAsync(*d_fb, 0, 4, ctx->stream));
    hipLaunchKernelGGL((tight_boxes_kernel<Node>), dim3((n + 255u) / 256u), dim3(256), 0, ctx->stream, sc.instances, n, sc.meshes, sc.n_meshes,
                       sc.bvh_nodes, sc.n_bvh_nodes, static_cast<const Node*>(a->user_tlas), a->user_n_nodes, a->boxes, *d_fb);
    return VD_OK;
}
// ... and what follows the build or the refit behind them: the count comes back (blocks), and the accel walks its private top
// level when every instance qualified, the scene's own otherwise.
template <bool WIDE>
int adopt_tight_tlas(VdCtx* ctx, VdTraceAccel* a, const unsigned* d_fb) {
    using Node = std::conditional_t<WIDE, VdTlasNodeWide, VdTlasNode>;
    SceneOf<WIDE>& sc = accel_scene<WIDE>(a);
    VD_HIP_CHECK(ctx, hipGetLastError());
    unsigned h_fallback = 0;
    VD_HIP_CHECK(ctx, hipMemcpyAsync(&h_fallback, d_fb, 4, hipMemcpyDeviceToHost, ctx->stream));
    VD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    a->tight_fallbacks = h_fallback;
    if (h_fallback) { sc.tlas_nodes = static_cast<const Node*>(a->user_tlas); sc.n_tlas_nodes = a->user_n_nodes; }      // declined: the reference's visit order is the only exact one here
    else { sc.tlas_nodes = static_cast<const Node*>(a->tight); sc.n_tlas_nodes = a->tight_mode == 2u ? 2u * sc.n_instances : 2u * sc.n_instances + 1u; }
    return VD_OK;
}

// The private top level of a prepared scene (VD_OPT_TRACE_TIGHT_TLAS: 1 = agglomerative, 2 = LBVH; WIDE: always the LBVH), from the
// scene's instances as they are now.  Blocks (it reads back how many instances did not qualify); with any, the scene's own top level is walked.
template <bool WIDE>
int build_tight_tlas(VdCtx* ctx, VdTraceAccel* a) {
    const unsigned n = accel_scene<WIDE>(a).n_instances;
    unsigned* d_fb = nullptr;
    int rc = launch_tight_boxes<WIDE>(ctx, a, &d_fb);
    if (rc) return rc;
    if constexpr (WIDE) {
        if ((rc = vd_tlas_lbvh_from_boxes_wide(ctx, a->boxes, n, static_cast<VdTlasNodeWide*>(a->tight), a->lbvh))) return rc;
    } else if (a->tight_mode == 2u) {
        if ((rc = vd_tlas_lbvh_from_boxes(ctx, a->boxes, n, static_cast<VdTlasNode*>(a->tight), a->lbvh))) return rc;
    } else {
        if ((rc = vd_tlas_build_from_boxes(ctx, a->boxes, n, static_cast<VdTlasNode*>(a->tight)))) return rc;
        hipLaunchKernelGGL(tight_root_kernel, dim3(1), dim3(64), 0, ctx->stream, static_cast<VdTlasNode*>(a->tight), n);
    }
    if ((rc = adopt_tight_tlas<WIDE>(ctx, a, d_fb))) return rc;
    a->refits = 0u;
    a->built_fallbacks = a->tight_fallbacks;
    return VD_OK;
}

// vd_trace_accel_refit_dev: new tight boxes into the leaves of the private tree as it stands, boxes bottom-up, same topology.
// A tree the AGGLOMERATIVE builder made while an instance did not qualify is rebuilt instead: that instance's box may have been
// everything, and the chain drops a cluster whose unions all reach 1e30 (tlas.hip, refit) - its tree cannot carry the scene.
template <bool WIDE>
int refit_tight_tlas(VdCtx* ctx, VdTraceAccel* a) {
    if (a->tight_mode == 1u && a->built_fallbacks) return build_tight_tlas<WIDE>(ctx, a);
    unsigned* d_fb = nullptr;
    int rc = launch_tight_boxes<WIDE>(ctx, a, &d_fb);
    if (rc) return rc;
    if ((rc = vd_tlas_refit_from_boxes(ctx, a->boxes, accel_scene<WIDE>(a).n_instances, a->tight, WIDE, &a->refit))) return rc;
    if ((rc = adopt_tight_tlas<WIDE>(ctx, a, d_fb))) return rc;
    ++a->refits;
    return VD_OK;
}

// de-index every mesh's leaves into `tris`; gridDim.y carries the mesh: 65 535 per launch
template <typename S>
void launch_prepare_tris(VdCtx* ctx, const S& s, float* tris, unsigned* err) {
    for (unsigned m0 = 0; m0 < s.n_meshes; m0 += 65535u)
        hipLaunchKernelGGL(prepare_tris_kernel, dim3(256, std::min(s.n_meshes - m0, 65535u)), dim3(256), 0, ctx->stream, s.meshes + m0,
                           s.vertices, s.indices, s.n_indices, s.n_vertices, tris, err);
}

// everything a VdTraceAccel owns, and the handle itself - when the stream no longer uses any of it
void accel_free(VdCtx* ctx, VdTraceAccel* a) {
    (void)hipStreamSynchronize(ctx->stream);
    if (a->tris) (void)hipFree(a->tris);
    if (a->tight) (void)hipFree(a->tight);
    if (a->boxes) (void)hipFree(a->boxes);
    if (a->lbvh) (void)hipFree(a->lbvh);
    if (a->refit.state) (void)hipFree(a->refit.state);
    delete a;
}

int fail_named(VdCtx* ctx, const char* name, const char* text) {
    snprintf(ctx->err, sizeof(ctx->err), "%s: %s", name, text);
    return VD_ERR_INVALID_ARG;
}
template <typename S> bool scene_ok(const S* s) {
    return s && s->tlas_nodes && s->instances && s->meshes && s->bvh_nodes && s->vertices && s->indices && s->n_meshes &&
           s->n_tlas_nodes && s->n_instances;
}

// vd_trace_prepare_dev / vd_trace_prepare_wide_dev: validate, de-index every leaf (no triangle limit), and - with
// VD_OPT_TRACE_TIGHT_TLAS and an instance count the builder takes - the private top level.  Blocks.  Nothing is left behind on failure.
template <bool WIDE>
int trace_prepare(VdCtx* ctx, const SceneOf<WIDE>* d_scene, VdTraceAccel** out) {
    using Node = std::conditional_t<WIDE, VdTlasNodeWide, VdTlasNode>;
    constexpr const char* name = WIDE ? "vd_trace_prepare_wide" : "vd_trace_prepare";
    VdDeviceGuard vd_guard_(ctx);   // run on ctx->device whatever the calling thread's current device is
    if (!ctx || !out) return VD_ERR_INVALID_ARG;
    *out = nullptr;
    if (!scene_ok(d_scene) || d_scene->n_indices == 0u || d_scene->n_vertices == 0u) return fail_named(ctx, name, "incomplete scene");
    if (WIDE && d_scene->n_tlas_nodes > 2u * VD_TLAS_WIDE_MAX_INSTANCES + 1u)
        return fail_named(ctx, name, "more than 2 * VD_TLAS_WIDE_MAX_INSTANCES + 1 top-level nodes");
    VdTraceAccel* a = new (std::nothrow) VdTraceAccel();
    if (!a) return VD_ERR_OOM;
    a->wide = WIDE; a->owner = ctx;
    if constexpr (WIDE) a->wscene = *d_scene; else a->scene = *d_scene;
    const size_t n_tri = d_scene->n_indices / 3u;
    auto oom = [&](const char* what) { accel_free(ctx, a); snprintf(ctx->err, sizeof(ctx->err), "%s: %s", name, what); return VD_ERR_OOM; };
    if (hipMalloc(reinterpret_cast<void**>(&a->tris), 36 * n_tri + 64) != hipSuccess) { a->tris = nullptr; (void)hipGetLastError(); return oom("triangle array"); }
    int rc = vd_ensure(ctx, &ctx->scratch, &ctx->scratch_bytes, 256);
    if (rc) { accel_free(ctx, a); return rc; }
    unsigned* d_flag = reinterpret_cast<unsigned*>(ctx->scratch);
    (void)hipMemsetAsync(d_flag, 0, 4, ctx->stream);
    (void)hipMemsetAsync(a->tris, 0, 36 * n_tri + 64, ctx->stream);      // index ranges no mesh covers
    launch_prepare_tris(ctx, *d_scene, a->tris, d_flag);
    hipError_t e = hipMemcpyAsync(ctx->host_pinned, d_flag, 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess || ctx->host_pinned[0]) {
        accel_free(ctx, a);
        if (e != hipSuccess) VD_FAIL(ctx, VD_ERR_HIP, hipGetErrorString(e));
        return fail_named(ctx, name, "a mesh's index range or a vertex index lies outside the scene's buffers");
    }
    a->user_tlas = d_scene->tlas_nodes; a->user_n_nodes = d_scene->n_tlas_nodes;
    const long long tight = ctx->option(VD_OPT_TRACE_TIGHT_TLAS, 0);
    const unsigned n = d_scene->n_instances;
    const unsigned n_max = WIDE ? VD_TLAS_WIDE_MAX_INSTANCES : (tight == 2 ? VD_TLAS_MAX_INSTANCES - 1u : VD_TLAS_MAX_INSTANCES);
    if (tight != 0 && n >= 2u && n <= n_max) {
        a->tight_mode = WIDE || tight == 2 ? 2u : 1u;      // wide: the agglomerative chain takes seconds at these sizes
        const size_t lbvh_bytes = vd_lbvh_work_bytes(n);
        bool good = hipMalloc(reinterpret_cast<void**>(&a->boxes), 24 * (size_t)n + 16) == hipSuccess &&       // (not in the context's scratch: the agglomerative builder lays that out for itself)
                    hipMalloc(&a->tight, sizeof(Node) * (2 * (size_t)n + 1)) == hipSuccess &&
                    (a->tight_mode != 2u || hipMalloc(reinterpret_cast<void**>(&a->lbvh), lbvh_bytes) == hipSuccess);
        if (good) good = hipMemsetAsync(a->tight, 0, sizeof(Node) * (2 * (size_t)n + 1), ctx->stream) == hipSuccess;      // slots a builder leaves unused read as leaves nobody reaches
        else (void)hipGetLastError();
        const int rc_t = good ? build_tight_tlas<WIDE>(ctx, a) : VD_ERR_OOM;
        if (rc_t) {
            if (rc_t == VD_ERR_OOM) return oom("the private top level (VD_OPT_TRACE_TIGHT_TLAS) could not be allocated");
            accel_free(ctx, a);
            return rc_t;
        }
    }
    *out = a;
    return VD_OK;
}

// host-pointer form of a trace call: the six buffers and the rays staged in, the records out
template <bool WIDE>
int trace_host(VdCtx* ctx, const SceneOf<WIDE>* scene, const VdRay* rays, uint32_t n_rays, VdHit* out) {
    using Node = std::conditional_t<WIDE, VdTlasNodeWide, VdTlasNode>;
    enum { kNodes, kInst, kMeshes, kBvh, kVerts, kIdx, kRays, kOut, kBlobs };
    VdBlob b[kBlobs] = {{scene->tlas_nodes, (size_t)scene->n_tlas_nodes * sizeof(Node), 256, nullptr},
                        {scene->instances, (size_t)scene->n_instances * sizeof(VdInstance), 256, nullptr},
                        {scene->meshes, (size_t)scene->n_meshes * sizeof(VdMeshInfo), 256, nullptr},
                        {scene->bvh_nodes, (size_t)scene->n_bvh_nodes * sizeof(VdBvhNode), 256, nullptr},
                        {scene->vertices, (size_t)scene->n_vertices * 12, 256, nullptr},
                        {scene->indices, (size_t)scene->n_indices * 4, 256, nullptr},
                        {rays, (size_t)n_rays * sizeof(VdRay), 256, nullptr},
                        {nullptr, (size_t)n_rays * sizeof(VdHit), 256, nullptr}};
    int rc = vd_stage_blobs(ctx, b, kBlobs);
    if (rc) return rc;
    auto d = *scene;
    d.tlas_nodes = static_cast<const Node*>(b[kNodes].dev);
    d.instances = static_cast<const VdInstance*>(b[kInst].dev);
    d.meshes = static_cast<const VdMeshInfo*>(b[kMeshes].dev);
    d.bvh_nodes = static_cast<const VdBvhNode*>(b[kBvh].dev);
    d.vertices = static_cast<const float*>(b[kVerts].dev);
    d.indices = static_cast<const uint32_t*>(b[kIdx].dev);
    rc = launch_trace<WIDE>(ctx, &d, nullptr, static_cast<const VdRay*>(b[kRays].dev), n_rays, static_cast<VdHit*>(b[kOut].dev));
    return rc ? rc : vd_fetch_blob(ctx, out, &b[kOut]);
}

// What every vd_trace* walker does: the device guard, the context, the scene (`name`: no_scene when it is missing or incomplete -
// every wide form words that as vd_trace_wide does, and refuses more nodes than the wide layout is specified for), nothing to
// do without rays, rays and a place for the result (`name`: null rays/out), and the call - staged when the pointers are the host's.
// Exactly one of out / any is the result; tris: the prepared leaves of vd_trace_*prepared_dev.
template <bool WIDE, bool HOST = false>
int trace_entry(VdCtx* ctx, const char* name, const char* no_scene, const SceneOf<WIDE>* sc, const float* tris, const VdRay* rays, uint32_t n_rays,
                VdHit* out, uint32_t* any) {
    VdDeviceGuard vd_guard_(ctx);   // run on ctx->device whatever the calling thread's current device is
    if (!ctx) return VD_ERR_INVALID_ARG;
    if (!scene_ok(sc)) return fail_named(ctx, WIDE ? "vd_trace_wide" : name, no_scene);
    if (WIDE && sc->n_tlas_nodes > 2u * VD_TLAS_WIDE_MAX_INSTANCES + 1u)
        VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_trace_wide: more than 2 * VD_TLAS_WIDE_MAX_INSTANCES + 1 top-level nodes");
    if (n_rays == 0) return VD_OK;
    if (!rays || (!out && !any)) return fail_named(ctx, name, "null rays/out");
    if constexpr (HOST) return trace_host<WIDE>(ctx, sc, rays, n_rays, out);
    else return launch_trace<WIDE>(ctx, sc, tris, rays, n_rays, out, any);
}

// vd_traverse_iter* / vd_traverse*: one mesh, one ray per lane; `recursive` picks the walk (traverse_rec_kernel, from t0) and
// `host` the form: the mesh and the rays staged in (n_vert vertices, n_tri triangles), the distances out.
int traverse_entry(VdCtx* ctx, bool recursive, bool host, float t0, const VdBvhNode* nodes, uint32_t n_nodes, const float* verts_xyz, uint32_t n_vert,
                   const uint32_t* indices, uint32_t n_tri, const VdRay* rays, uint32_t n_rays, float* out_dist) {
    VdDeviceGuard vd_guard_(ctx);   // run on ctx->device whatever the calling thread's current device is
    const char* name = host ? "vd_traverse[_iter]" : recursive ? "vd_traverse" : "vd_traverse_iter";
    if (!ctx) return VD_ERR_INVALID_ARG;
    if (!nodes || n_nodes == 0 || !verts_xyz || !indices) return fail_named(ctx, name, "incomplete mesh");
    if (n_rays == 0) return VD_OK;
    if (!rays || !out_dist) return fail_named(ctx, name, "null rays/out");
    VdBlob b[5] = {{nodes, (size_t)n_nodes * sizeof(VdBvhNode), 256, nullptr}, {verts_xyz, (size_t)n_vert * 12, 256, nullptr},
                   {indices, (size_t)n_tri * 12, 256, nullptr}, {rays, (size_t)n_rays * sizeof(VdRay), 256, nullptr},
                   {nullptr, (size_t)n_rays * 4, 256, nullptr}};
    int rc = host ? vd_stage_blobs(ctx, b, 5) : VD_OK;
    if (rc) return rc;
    const VdBvhNode* d_nodes = host ? static_cast<const VdBvhNode*>(b[0].dev) : nodes;
    const float* d_verts = host ? static_cast<const float*>(b[1].dev) : verts_xyz;
    const uint32_t* d_indices = host ? static_cast<const uint32_t*>(b[2].dev) : indices;
    const VdRay* d_rays = host ? static_cast<const VdRay*>(b[3].dev) : rays;
    float* d_out = host ? static_cast<float*>(b[4].dev) : out_dist;
    if ((rc = vd_ensure(ctx, &ctx->scratch, &ctx->scratch_bytes, 256))) return rc;
    unsigned* d_flag = reinterpret_cast<unsigned*>(ctx->scratch);
    vd_time_begin(ctx);
    VD_HIP_CHECK(ctx, hipMemsetAsync(d_flag, 0, 4, ctx->stream));
    if (recursive) hipLaunchKernelGGL(traverse_rec_kernel, dim3((n_rays + 63u) / 64u), dim3(64), 0, ctx->stream, d_nodes, d_verts, d_indices, d_rays,
                                      n_rays, t0, d_out, d_flag);
    else hipLaunchKernelGGL(traverse_iter_kernel, dim3((n_rays + 63u) / 64u), dim3(64), 0, ctx->stream, d_nodes, d_verts, d_indices, d_rays,
                            n_rays, d_out, d_flag);
    vd_time_end(ctx);
    VD_HIP_CHECK(ctx, hipGetLastError());
    VD_HIP_CHECK(ctx, hipMemcpyAsync(ctx->host_pinned, d_flag, 4, hipMemcpyDeviceToHost, ctx->stream));
    VD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->host_pinned[0]) VD_FAIL(ctx, VD_ERR_STACK_OVERFLOW, recursive ? "vd_traverse: traversal stack (128 pending right children per ray) exceeded"
                                                                           : "vd_traverse_iter: traversal stack (128 entries per ray) exceeded");
    return host ? vd_fetch_blob(ctx, out_dist, &b[4]) : VD_OK;
}

}  // namespace

extern "C" {

#ifdef VD_TUNING
// tuning build only: {outer iterations, stepping-loop iterations, stepping lanes (64 bit), leaf / entry / TLAS-interior lane-steps} of the last trace call
// tuning build only: the last trace call's timeline in 2 ms slots: out[0..22] waves that ended in the slot, out[23..45] stepping iterations done in it
int vd_debug_trace_timeline(VdCtx* ctx, uint32_t* out /*[46]*/) {
    VdDeviceGuard vd_guard_(ctx);
    if (!ctx || !out || !ctx->scratch) return VD_ERR_INVALID_ARG;
    unsigned h[64];
    if (hipMemcpy(h, ctx->scratch, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return VD_ERR_HIP;
    for (int k = 0; k < 46; ++k) out[k] = h[18 + k];
    return VD_OK;
}
int vd_debug_trace_counters(VdCtx* ctx, uint64_t* out /*[11]*/) {
    VdDeviceGuard vd_guard_(ctx);
    if (!ctx || !out || !ctx->scratch) return VD_ERR_INVALID_ARG;
    unsigned h[16];
    if (hipMemcpy(h, ctx->scratch, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return VD_ERR_HIP;
    out[0] = h[4]; out[1] = h[5]; out[2] = (uint64_t)h[6] | ((uint64_t)h[7] << 32); out[3] = h[8]; out[4] = h[9]; out[5] = h[10]; out[6] = h[11]; out[7] = h[12]; out[8] = h[13]; out[9] = h[14]; out[10] = h[15];
    return VD_OK;
}
// tuning build only: the job supply of the last trace call (narrow or wide).  out[0] = waves that left the outer loop with nobody
// busy while their launch's supply was not exhausted (the supply rule: always 0), out[1] = launches the call ran as, out[2] = waves
// of the grid, out[3] = job slots, out[4] = jobs appended (ctl[0]; may exceed the slots when the list filled up), and for launch
// p = 1 .. 3: out[4 + p] = its supply counter (ctl[p]: positions drawn, the draws past the end included), out[8 + p] = the end of its
// supply (ctl[8 + p]; it begins at out[8 + p - 1], out[8] = 0).  A call of one launch leaves out[3..] zero.
int vd_debug_trace_fan(VdCtx* ctx, uint32_t* out /*[16]*/) {
    VdDeviceGuard vd_guard_(ctx);
    if (!ctx || !out || ctx->dbg_fan_phases == 0u) return VD_ERR_INVALID_ARG;
    const char* arena = reinterpret_cast<const char*>(ctx->dbg_fan_wide ? ctx->trace_wide : ctx->scratch);
    const size_t arena_bytes = ctx->dbg_fan_wide ? ctx->trace_wide_bytes : ctx->scratch_bytes;
    if (!arena || arena_bytes < 256 || (ctx->dbg_fan_phases > 1u && arena_bytes < ctx->dbg_fan_at + 256)) return VD_ERR_INVALID_ARG;
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) return VD_ERR_HIP;
    memset(out, 0, 16 * sizeof(uint32_t));
    unsigned h[16];
    if (hipMemcpy(h, arena, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return VD_ERR_HIP;
    out[0] = h[3]; out[1] = ctx->dbg_fan_phases; out[2] = ctx->dbg_fan_waves;
    if (ctx->dbg_fan_phases == 1u) return VD_OK;
    if (hipMemcpy(h, arena + ctx->dbg_fan_at, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return VD_ERR_HIP;
    out[3] = ctx->dbg_fan_cap; out[4] = h[0];
    for (unsigned p = 1; p < 4u; ++p) { out[4 + p] = h[p]; out[8 + p] = h[8 + p]; }
    return VD_OK;
}
#endif

// The walkers (trace_entry): what differs is the name in the messages, the node type, whose pointers these are, and closest hit / any hit.
int vd_trace_dev(VdCtx* ctx, const VdTraceScene* d_scene, const VdRay* d_rays, uint32_t n_rays, VdHit* d_out) {
    return trace_entry<false>(ctx, "vd_trace", "incomplete scene", d_scene, nullptr, d_rays, n_rays, d_out, nullptr);
}
int vd_trace_any_dev(VdCtx* ctx, const VdTraceScene* d_scene, const VdRay* d_rays, uint32_t n_rays, uint32_t* d_out_hit) {
    return trace_entry<false>(ctx, "vd_trace_any", "incomplete scene", d_scene, nullptr, d_rays, n_rays, nullptr, d_out_hit);
}
int vd_trace_prepared_dev(VdCtx* ctx, const VdTraceAccel* accel, const VdRay* d_rays, uint32_t n_rays, VdHit* d_out) {
    if (accel && accel->wide) return trace_entry<true>(ctx, "vd_trace_prepared", "null accel", &accel->wscene, accel->tris, d_rays, n_rays, d_out, nullptr);
    return trace_entry<false>(ctx, "vd_trace_prepared", "null accel", accel ? &accel->scene : nullptr, accel ? accel->tris : nullptr, d_rays, n_rays, d_out, nullptr);
}
int vd_trace_any_prepared_dev(VdCtx* ctx, const VdTraceAccel* accel, const VdRay* d_rays, uint32_t n_rays, uint32_t* d_out_hit) {
    if (accel && accel->wide) return trace_entry<true>(ctx, "vd_trace_any_prepared", "null accel", &accel->wscene, accel->tris, d_rays, n_rays, nullptr, d_out_hit);
    return trace_entry<false>(ctx, "vd_trace_any_prepared", "null accel", accel ? &accel->scene : nullptr, accel ? accel->tris : nullptr, d_rays, n_rays, nullptr, d_out_hit);
}
int vd_trace(VdCtx* ctx, const VdTraceScene* scene, const VdRay* rays, uint32_t n_rays, VdHit* out) {
    return trace_entry<false, true>(ctx, "vd_trace", "incomplete scene", scene, nullptr, rays, n_rays, out, nullptr);
}
int vd_trace_wide_dev(VdCtx* ctx, const VdTraceSceneWide* d_scene, const VdRay* d_rays, uint32_t n_rays, VdHit* d_out) {
    return trace_entry<true>(ctx, "vd_trace_wide", "incomplete scene", d_scene, nullptr, d_rays, n_rays, d_out, nullptr);
}
int vd_trace_any_wide_dev(VdCtx* ctx, const VdTraceSceneWide* d_scene, const VdRay* d_rays, uint32_t n_rays, uint32_t* d_out_hit) {
    return trace_entry<true>(ctx, "vd_trace_any_wide", "incomplete scene", d_scene, nullptr, d_rays, n_rays, nullptr, d_out_hit);
}
int vd_trace_wide(VdCtx* ctx, const VdTraceSceneWide* scene, const VdRay* rays, uint32_t n_rays, VdHit* out) {
    return trace_entry<true, true>(ctx, "vd_trace_wide", "incomplete scene", scene, nullptr, rays, n_rays, out, nullptr);
}

int vd_trace_prepare_dev(VdCtx* ctx, const VdTraceScene* d_scene, VdTraceAccel** out) { return trace_prepare<false>(ctx, d_scene, out); }
int vd_trace_prepare_wide_dev(VdCtx* ctx, const VdTraceSceneWide* d_scene, VdTraceAccel** out) { return trace_prepare<true>(ctx, d_scene, out); }

int vd_trace_accel_info(const VdTraceAccel* accel, VdTraceAccelInfo* out) {
    if (!accel || !out) return VD_ERR_INVALID_ARG;
    if (accel->wide) VD_FAIL(accel->owner, VD_ERR_INVALID_ARG, "vd_trace_accel_info: the accel was made by vd_trace_prepare_wide_dev: use vd_trace_accel_info_wide");
    memset(out, 0, sizeof(*out));
    out->tight_tlas = (accel->tight && accel->scene.tlas_nodes == accel->tight) ? accel->tight_mode : 0u;
    out->n_tlas_nodes = accel->scene.n_tlas_nodes;
    out->tight_fallback_instances = accel->tight_fallbacks;
    out->triangle_bytes = 36ull * (accel->scene.n_indices / 3u);
    out->d_tlas_nodes = accel->scene.tlas_nodes;
    return VD_OK;
}
int vd_trace_accel_info_wide(const VdTraceAccel* accel, VdTraceAccelInfoWide* out) {
    if (!accel || !out) return VD_ERR_INVALID_ARG;
    if (!accel->wide) VD_FAIL(accel->owner, VD_ERR_INVALID_ARG, "vd_trace_accel_info_wide: the accel was made by vd_trace_prepare_dev: use vd_trace_accel_info");
    memset(out, 0, sizeof(*out));
    out->tight_tlas = (accel->tight && accel->wscene.tlas_nodes == accel->tight) ? accel->tight_mode : 0u;
    out->n_tlas_nodes = accel->wscene.n_tlas_nodes;
    out->tight_fallback_instances = accel->tight_fallbacks;
    out->refits_since_build = accel->refits;
    out->triangle_bytes = 36ull * (accel->wscene.n_indices / 3u);
    out->d_tlas_nodes = accel->wscene.tlas_nodes;
    return VD_OK;
}

int vd_trace_accel_update_dev(VdCtx* ctx, VdTraceAccel* accel) {
    VdDeviceGuard vd_guard_(ctx);
    if (!ctx || !accel) return VD_ERR_INVALID_ARG;
    if (!accel->tight) return VD_OK;          // the scene's own top level is walked: the host refits that one (vd_tlas_refit_dev)
    ctx->fan_forget(accel->tight);
    return accel->wide ? build_tight_tlas<true>(ctx, accel) : build_tight_tlas<false>(ctx, accel);
}

int vd_trace_accel_refit_dev(VdCtx* ctx, VdTraceAccel* accel) {
    VdDeviceGuard vd_guard_(ctx);
    if (!ctx || !accel) return VD_ERR_INVALID_ARG;
    if (!accel->tight) return VD_OK;          // as above
    ctx->fan_forget(accel->tight);
    return accel->wide ? refit_tight_tlas<true>(ctx, accel) : refit_tight_tlas<false>(ctx, accel);
}

int vd_trace_accel_update_geometry_dev(VdCtx* ctx, VdTraceAccel* accel) {
    VdDeviceGuard vd_guard_(ctx);
    if (!ctx || !accel) return VD_ERR_INVALID_ARG;
    const uint32_t n_indices = accel->wide ? accel->wscene.n_indices : accel->scene.n_indices;
    unsigned* d_ignored = reinterpret_cast<unsigned*>(accel->tris + 9 * (size_t)(n_indices / 3u));      // the array's slack: prepare validated, nobody reads this word
    if (accel->wide) launch_prepare_tris(ctx, accel->wscene, accel->tris, d_ignored);
    else launch_prepare_tris(ctx, accel->scene, accel->tris, d_ignored);
    VD_HIP_CHECK(ctx, hipGetLastError());
    return VD_OK;
}

int vd_trace_release(VdCtx* ctx, VdTraceAccel* accel) {
    VdDeviceGuard vd_guard_(ctx);
    if (!ctx || !accel) return VD_ERR_INVALID_ARG;
    if (accel->tight) ctx->fan_forget(accel->tight);
    accel_free(ctx, accel);
    return VD_OK;
}

int vd_shadow_rays_dev(VdCtx* ctx, const float* d_positions, const float* d_normals, uint32_t n_points, const float* light_position,
                       VdRay* d_rays) {
    VdDeviceGuard vd_guard_(ctx);   // run on ctx->device whatever the calling thread's current device is
    if (!ctx) return VD_ERR_INVALID_ARG;
    if (n_points == 0) return VD_OK;
    if (!d_positions || !d_normals || !light_position || !d_rays) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_shadow_rays: null pointer");
    const bool range = ctx->option(VD_OPT_TRACE_RAY_RANGE, 0) == 1;      // the open segment from the offset point to the light: t in (0, 1)
    hipLaunchKernelGGL(shadow_rays_kernel, dim3((n_points + 255) / 256), dim3(256), 0, ctx->stream, d_positions, d_normals, n_points,
                       light_position[0], light_position[1], light_position[2], 0.0f, range ? 1.0f : 0.0f, d_rays);
    VD_HIP_CHECK(ctx, hipGetLastError());
    return VD_OK;
}

int vd_primary_rays_dev(VdCtx* ctx, const VdCameraUniform* camera, uint32_t width, uint32_t height, VdRay* d_rays) {
    VdDeviceGuard vd_guard_(ctx);   // run on ctx->device whatever the calling thread's current device is
    if (!ctx) return VD_ERR_INVALID_ARG;
    if (!camera) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_primary_rays: null camera");
    const uint64_t n = (uint64_t)width * height;
    if (n == 0) return VD_OK;
    if (!d_rays) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_primary_rays: null rays");
    if (n > 0xffffff00ull) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_primary_rays: width * height does not fit 32 bits");
    Mat4 c2w;
    for (int k = 0; k < 16; ++k) c2w.m[k] = camera->clip_to_world[k];
    hipLaunchKernelGGL(primary_rays_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, c2w, width, height, (unsigned)n, 0.0f,
                       ctx->option(VD_OPT_TRACE_RAY_RANGE, 0) == 1 ? VD_MAX_DIST : 0.0f, d_rays);      // under the option: the whole half-line
    VD_HIP_CHECK(ctx, hipGetLastError());
    return VD_OK;
}

int vd_primary_rays(VdCtx* ctx, const VdCameraUniform* camera, uint32_t width, uint32_t height, VdRay* rays) {
    VdDeviceGuard vd_guard_(ctx);   // run on ctx->device whatever the calling thread's current device is
    if (!ctx) return VD_ERR_INVALID_ARG;
    const uint64_t n = (uint64_t)width * height;
    if (n && !rays) VD_FAIL(ctx, VD_ERR_INVALID_ARG, "vd_primary_rays: null rays");
    VdBlob b = {nullptr, (size_t)n * sizeof(VdRay), 256, nullptr};
    int rc = vd_stage_blobs(ctx, &b, 1);
    if (rc) return rc;
    rc = vd_primary_rays_dev(ctx, camera, width, height, static_cast<VdRay*>(b.dev));
    if (rc || n == 0) return rc;
    return vd_fetch_blob(ctx, rays, &b);
}

int vd_traverse_iter_dev(VdCtx* ctx, const VdBvhNode* d_nodes, uint32_t n_nodes, const float* d_verts_xyz, const uint32_t* d_indices,
                         const VdRay* d_rays, uint32_t n_rays, float* d_out_dist) {
    return traverse_entry(ctx, false, false, 0.0f, d_nodes, n_nodes, d_verts_xyz, 0, d_indices, 0, d_rays, n_rays, d_out_dist);
}
int vd_traverse_dev(VdCtx* ctx, const VdBvhNode* d_nodes, uint32_t n_nodes, const float* d_verts_xyz, const uint32_t* d_indices,
                    const VdRay* d_rays, uint32_t n_rays, float t0, float* d_out_dist) {
    return traverse_entry(ctx, true, false, t0, d_nodes, n_nodes, d_verts_xyz, 0, d_indices, 0, d_rays, n_rays, d_out_dist);
}
int vd_traverse_iter(VdCtx* ctx, const VdBvhNode* nodes, uint32_t n_nodes, const float* verts_xyz, uint32_t n_vert,
                     const uint32_t* indices, uint32_t n_tri, const VdRay* rays, uint32_t n_rays, float* out_dist) {
    return traverse_entry(ctx, false, true, 0.0f, nodes, n_nodes, verts_xyz, n_vert, indices, n_tri, rays, n_rays, out_dist);
}
int vd_traverse(VdCtx* ctx, const VdBvhNode* nodes, uint32_t n_nodes, const float* verts_xyz, uint32_t n_vert,
                const uint32_t* indices, uint32_t n_tri, const VdRay* rays, uint32_t n_rays, float t0, float* out_dist) {
    return traverse_entry(ctx, true, true, t0, nodes, n_nodes, verts_xyz, n_vert, indices, n_tri, rays, n_rays, out_dist);
}

}  // extern "C"
