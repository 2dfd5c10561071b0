"""vd_trace* past the 128 stack entries a lane holds, and past the first 1 Ki entries of the global-memory pass behind them;
vd_traverse_iter* / vd_traverse* on both sides of their 128-entry return.  Everything is held against the CPU oracle, bytes for
bytes (no tolerance anywhere), and every case first asserts ON THE ORACLE'S OWN DEPTHS that it is the case it claims to be.

Depth here is the oracle's SHARED FAR-ONLY depth of a ray (oracle/vd_oracle.h, vd_ref_trace_depths): pending TLAS + BLAS entries
on one stack, far children only - the unit include/voidin_abi.h states the 128 in.  A ray of depth d is served by the first
pass iff d <= 128, and by the iteration of launch_trace's `cap` loop (1 Ki, 4 Ki, 16 Ki, 64 Ki entries behind the 128) whose
class it falls in: d <= 1 152, 4 224, 16 512, 65 664.  A lane's stack has two more seams below that: entries 0..23 in LDS,
24..127 in registers (kLdsStack, 2 * kStack in trace.hip).

The chain lengths below were read off the oracle's output (chain_scene(N): depth N + 6, the small sphere's own BLAS on top of
N - 1 TLAS entries; chain_blas_scene(n): n - 2; chain_mixed_scene(N, n): N + n - 4) and every test asserts the depth it gets."""
import numpy as np
import pytest

from chain_scenes import chain_blas_mesh, chain_blas_scene, chain_mixed_scene, chain_rays, chain_scene
from voidin_amd import abi
from voidin_amd.runtime import Context, VoidinError

pytestmark = pytest.mark.gpu

CLASS_TOP = (128, 1152, 4224, 16512, 65664)      # 128 + 0, 1 Ki, 4 Ki, 16 Ki, 64 Ki


def _class_of(depth):
    """0: the first pass; k >= 1: the k-th iteration of the second pass's cap loop."""
    return np.searchsorted(np.array(CLASS_TOP), depth, side="left")


def _scene(oracle, kind, length):
    """(scene, x beyond its far end)"""
    if kind == "tlas":
        return chain_scene(oracle, length), length + 50.0
    if kind == "blas":
        return chain_blas_scene(oracle, length), length + 50.0
    return chain_mixed_scene(oracle, *length), max(length) + 50.0


def _walks(ctx, ctx_options, scene, rays, want, tag, fans=(1,), modes=("plain", "indexed", "prepared")):
    """vd_trace* and vd_trace_any* over device buffers on each walk; records and flags equal to the oracle's, bytes."""
    import torch
    n = len(rays)
    ds = ctx.device_scene(scene)
    d_rays, d_hits = ctx.upload(rays), ctx.empty(n * 16)
    d_any = torch.zeros(n, dtype=torch.int32, device="cuda")
    acc = ctx.trace_prepare(ds) if "prepared" in modes else None
    want_b = np.ascontiguousarray(want).tobytes()
    try:
        for fan in fans:
            ctx_options("trace.fan", fan)
            for mode in modes:
                ctx_options("trace.auto_prepare", 0 if mode == "indexed" else None)
                d_hits.zero_(); d_any.zero_()
                if mode == "prepared":
                    ctx.trace_prepared_dev(acc, d_rays, n, d_hits); ctx.trace_any_prepared_dev(acc, d_rays, n, d_any)
                else:
                    ctx.trace_dev(ds, d_rays, n, d_hits); ctx.trace_any_dev(ds, d_rays, n, d_any)
                got = d_hits.cpu().numpy()[: n * 16].view(abi.HIT)
                if got.tobytes() != want_b:
                    bad = np.nonzero((got.view(np.uint32).reshape(n, 4) != np.ascontiguousarray(want).view(np.uint32).reshape(n, 4)).any(axis=1))[0]
                    raise AssertionError(f"{tag} fan {fan} {mode}: {len(bad)} records differ, first ray {bad[0]}: got {got[bad[0]]} want {want[bad[0]]}")
                assert np.array_equal(d_any.cpu().numpy().astype(np.uint32), want["hit"]), (tag, fan, mode, "occlusion flags")
    finally:
        if acc is not None:
            acc.close()
        ctx_options("trace.fan", None); ctx_options("trace.auto_prepare", None)


# (kind, seam) -> the lengths whose deepest ray runs through lo..hi, one step each
def _sweep_lengths(kind, lo, hi):
    if kind == "tlas":
        return [d - 6 for d in range(lo, hi + 1)]
    if kind == "blas":
        return [d + 2 for d in range(lo, hi + 1)]
    n_leaves = {20: 10, 120: 64, 1144: 600}[lo]         # the seam lies INSIDE the nearest instance, above n_leaves - 1 TLAS entries
    return [(n_leaves, d - n_leaves + 4) for d in range(lo, hi + 1)]


@pytest.mark.parametrize("kind", ["tlas", "blas", "mixed"])
@pytest.mark.parametrize("lo,hi,seam", [(20, 28, 24), (120, 136, 128), (1144, 1160, 1152)])
def test_seam_sweep(ctx, ctx_options, oracle, kind, lo, hi, seam):
    """Chain lengths one apart, so that the deepest ray of a call sits below, ON and above each seam of a lane's stack: LDS /
    registers at 24 (no second pass), registers / global slab at 128 (the last entry that fits, the first ray that is walked
    again), the slab's first size at 128 + 1 Ki (the last entry of iteration 1, the first ray that needs iteration 2).  In the
    mixed scene the seam is crossed inside an instance entered with blas_base > 0 and the entries are popped back across it
    into the TLAS entries underneath."""
    covered = []
    for length in _sweep_lengths(kind, lo, hi):
        scene, far_x = _scene(oracle, kind, length)
        rays, far_side, cheap = chain_rays(2_000, far_x, seed=seam)
        want, _, depth = oracle.trace(scene, rays, threads=16, depths=True)
        top = int(depth.max())
        at_top = depth == top
        assert want["hit"][at_top].sum() > 0, (kind, length, "every deepest ray misses")
        assert (depth[cheap] == 0).all()                 # the rays that leave at once
        covered.append(top)
        _walks(ctx, ctx_options, scene, rays, want, f"{kind} {length} depth {top}")
    print(f"\nseam {seam} {kind}: deepest far-only depth per call {covered}")
    assert covered == list(range(lo, hi + 1)), "the sweep does not step through every depth across the seam"
    assert {seam - 1, seam, seam + 1} <= set(covered)


REGROW = {
    "tlas 1400": ("tlas", 1400, 2), "tlas 4400": ("tlas", 4400, 3), "blas 1500": ("blas", 1500, 2),
    "blas 4300": ("blas", 4300, 3), "mixed 1000+400": ("mixed", (1000, 400), 2),
}


@pytest.mark.parametrize("case", list(REGROW))
def test_regrow(ctx, ctx_options, oracle, case):
    """Rays that need the 2nd and the 3rd iteration of the cap loop (4 Ki, 16 Ki entries behind the 128): control words zeroed
    again, the list made again from the bitmap, every listed ray walked again from its start, the slab freed and allocated
    larger in between, fewer waves than the first iteration had.  All three walks, closest hit and occlusion; and the occlusion
    walk stops (kDone) at a first accepted triangle that comes while more than 128 entries are pending."""
    kind, length, klass = REGROW[case]
    scene, far_x = _scene(oracle, kind, length)
    rays, far_side, cheap = chain_rays(2_000, far_x, seed=klass)
    want, _, depth, at_hit = oracle.trace(scene, rays, threads=16, first_hit=True)
    top = int(depth.max())
    deep = _class_of(depth) == klass
    print(f"\nregrow {case}: deepest {top}, rays per class {np.bincount(_class_of(depth), minlength=5).tolist()}, hits among class {klass}: {int(want['hit'][deep].sum())}")
    assert CLASS_TOP[klass - 1] < top <= CLASS_TOP[klass]
    assert want["hit"][deep].sum() > 0
    stops_deep = (want["hit"] == 1) & (at_hit != 0xFFFFFFFF) & (at_hit > 128)
    assert stops_deep.sum() > 0, "no ray whose first accepted triangle comes with more than 128 entries pending"
    _walks(ctx, ctx_options, scene, rays, want, case)


def _mixed_class_rays(n_leaves, n_rays, seed):
    """Rays along +x that start between two spheres of chain_scene(n_leaves), k spheres before its far end: only the k spheres
    ahead are pushed, so k sets the depth.  k from every class up to the chain's own, interleaved ray by ray."""
    rng = np.random.default_rng(seed)
    rays = np.zeros(n_rays, dtype=abi.RAY)
    ks = np.array([3, 60, 121, 122, 123, 124, 500, 1145, 1146, 1147, 1148, 3000, 4217, 4218, 4219, n_leaves + 5])
    k = ks[rng.integers(0, len(ks), n_rays)]
    rays["eye"] = (rng.random((n_rays, 3)).astype(np.float32) - np.float32(0.5)) * np.array([0.0, 0.5, 0.5], np.float32)
    rays["eye"][:, 0] = (n_leaves - k).astype(np.float32) - np.float32(0.5)
    rays["dir"] = np.array([1.0, 0.0, 0.0], np.float32)
    return rays


def test_regrow_with_every_class_in_one_call(ctx, ctx_options, oracle):
    """One call whose rays fall in all four classes a 4 400-leaf chain allows (fit in 128; need 1 Ki; 4 Ki; 16 Ki), interleaved,
    with depths right at 128 and at 1 152 / 4 224 among them: iteration 2 walks again - and rewrites - the rays iteration 1 had
    finished, iteration 3 those of both, and every record must still be the oracle's."""
    n_leaves = 4400
    scene = chain_scene(oracle, n_leaves)
    rays = _mixed_class_rays(n_leaves, 3_000, seed=5)
    want, _, depth = oracle.trace(scene, rays, threads=16, depths=True)
    klass = _class_of(depth)
    hits_per_class = [int(want["hit"][klass == c].sum()) for c in range(4)]
    print(f"\nevery class in one call: depths {sorted(set(depth.tolist()))}, rays per class {np.bincount(klass, minlength=4).tolist()}, hits per class {hits_per_class}")
    assert klass.max() == 3 and min(hits_per_class) > 0
    assert {127, 128, 129, 1151, 1152, 1153, 4223, 4224, 4225} <= set(depth.tolist())
    _walks(ctx, ctx_options, scene, rays, want, "every class")


def test_regrow_in_a_call_that_fans_out(ctx, ctx_options, oracle):
    """420 000 rays, 97 % of them leaving the scene at once, the deep ones in the 4 Ki class: the call fans out (trace.fan 3), so
    the bitmap is fed by the fan-out's first pass - by a fanned-out job under its ray's id - and the second pass runs its second
    iteration behind it."""
    scene, far_x = _scene(oracle, "tlas", 1400)
    n = 420_000
    rays, far_side, cheap = chain_rays(n, far_x, seed=420, cheap=0.97)
    want, _, depth = oracle.trace(scene, rays, threads=16, depths=True)
    deep = _class_of(depth) == 2
    print(f"\nfan-out: deepest {int(depth.max())}, rays per class {np.bincount(_class_of(depth), minlength=5).tolist()}, hits among class 2: {int(want['hit'][deep].sum())}")
    assert _class_of(depth).max() == 2 and want["hit"][deep].sum() > 0 and want["hit"].sum() > n // 100
    _walks(ctx, ctx_options, scene, rays, want, "fan-out", fans=(1, 3))


def test_deepest_chain_the_16_bit_layout_is_tested_at(ctx, ctx_options, oracle):
    """17 000 leaves: the 4th iteration (64 Ki entries per lane, 16 waves under the slab's 256 MB budget).  Plain walk only."""
    scene, far_x = _scene(oracle, "tlas", 17_000)
    rays, far_side, cheap = chain_rays(2_000, far_x, seed=17)
    want, _, depth = oracle.trace(scene, rays, threads=16, depths=True)
    deep = _class_of(depth) == 4
    print(f"\n17 000 leaves: deepest {int(depth.max())}, rays per class {np.bincount(_class_of(depth), minlength=5).tolist()}, hits among class 4: {int(want['hit'][deep].sum())}")
    assert CLASS_TOP[3] < int(depth.max()) <= CLASS_TOP[4] and want["hit"][deep].sum() > 0
    _walks(ctx, ctx_options, scene, rays, want, "17 000 leaves", modes=("plain",))


def test_state_carried_between_calls():
    """What one context keeps from call to call: the overflow bitmap (64 KiB = 524 288 rays at first, grown by vd_ensure, which
    frees and allocates), its "left clean" promise, and the slab.  In order, each call against the oracle: shallow; deep, 2 000
    rays (slab first allocated); deep, 600 000 rays (the bitmap grows while the previous call left it clean); deep, 1 100 001
    rays - not a multiple of 32 - whose LAST rays are deep (last bitmap word partly used); a 4 Ki-class call (slab regrown after
    use); the first shallow call again; and after every deep call an easy one (bitmap left clean).  Every output buffer is 256
    bytes longer than the call needs and the tail must come back untouched.

    launch_trace used to zero the grown bitmap only when its POINTER changed; a buffer that comes back at the address just freed
    kept an uninitialised upper half, and the listing kernel turned such bits into ray ids past n_rays.  What a fresh allocation
    holds is not under a test's control, so this sequence is not expected to fail on the code before that fix; it pins the
    sequence and the guard band, nothing more."""
    import torch
    from oracle import ref as oracle
    assert torch.cuda.is_available(), "gpu-marked test run without a GPU"
    shallow, far_a = chain_scene(oracle, 200), 250.0
    deeper, far_b = chain_scene(oracle, 1400), 1450.0
    GUARD = 256

    def deep_last(n, far_x, seed, cheap_share):
        rays, far_side, cheap = chain_rays(n, far_x, seed=seed, cheap=cheap_share)
        rays["eye"][-5:, 0], rays["eye"][-5:, 1:] = np.float32(-5.0), np.float32(0.0)      # the last rays: down the middle of the chain from its near end
        rays["dir"][-5:] = np.array([1.0, 0.0, 0.0], np.float32)
        far_side[-5:] = cheap[-5:] = False
        return rays, far_side, cheap

    c = Context(0)
    try:
        scenes = {}

        def call(name, scene, rays, klass):
            want, _, depth = oracle.trace(scene, rays, threads=16, depths=True)
            got_class = int(_class_of(depth).max())
            print(f"\nstate: {name}: {len(rays)} rays, deepest {int(depth.max())}, class {got_class}, deep rays {int((depth > 128).sum())}, hits among them {int(want['hit'][depth > 128].sum())}")
            assert got_class == klass
            if klass:
                assert want["hit"][_class_of(depth) == klass].sum() > 0
            if id(scene) not in scenes:
                scenes[id(scene)] = c.device_scene(scene)
            n = len(rays)
            d_rays = c.upload(rays)
            d_hits = torch.full((n * 16 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
            d_any = torch.full((n * 4 + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
            c.trace_dev(scenes[id(scene)], d_rays, n, d_hits)
            c.trace_any_dev(scenes[id(scene)], d_rays, n, d_any)
            h, a = d_hits.cpu().numpy(), d_any.cpu().numpy()
            assert (h[n * 16:] == 0xA5).all() and (a[n * 4:] == 0x5A).all(), f"{name}: wrote past the end of an output buffer"
            assert h[: n * 16].tobytes() == np.ascontiguousarray(want).tobytes(), name
            assert np.array_equal(a[: n * 4].view(np.uint32), want["hit"]), name
            return depth

        first, fs, ch = chain_rays(3_000, far_a, seed=1)
        first = first[fs | ch]                                    # nothing deep in it
        easy_small = first[:500]
        call("shallow", shallow, first, 0)
        r, fs, ch = deep_last(2_000, far_a, 2, 0.3)
        call("deep, slab first allocated", shallow, r, 1); call("easy after it", shallow, easy_small, 0)
        r, fs, ch = deep_last(600_000, far_a, 3, 0.97)
        call("deep, bitmap grows", shallow, r, 1); call("easy after it", shallow, r[fs | ch][:300_000], 0)
        r, fs, ch = deep_last(1_100_001, far_a, 4, 0.97)
        assert len(r) % 32 != 0
        d = call("deep, last word partly used", shallow, r, 1)
        assert (d[-5:] > 128).all()
        call("easy after it", shallow, r[fs | ch][:1_000_003], 0)
        r, fs, ch = deep_last(2_000, far_b, 5, 0.3)
        call("4 Ki class, slab regrown", deeper, r, 2); call("easy after it", deeper, r[fs | ch], 0)
        call("shallow again", shallow, first, 0)
    finally:
        c.close()


def _mesh_on_device(ctx, n_tris):
    nodes, verts, idx = chain_blas_mesh(n_tris)
    return (nodes, verts, idx), (ctx.upload(nodes), len(nodes), ctx.upload(verts.astype(np.float32)), ctx.upload(idx.astype(np.uint32)))


@pytest.mark.parametrize("walk", ["iter", "recursive"])
def test_traverse_returns_at_128_entries(ctx, oracle, walk):
    """vd_traverse_iter_dev / vd_traverse_dev document 128 entries and VD_ERR_STACK_OVERFLOW beyond.  One mesh, the BLAS chain,
    lengths one apart; which side of 128 a length is on is the ORACLE's statement (oracle/vd_oracle.h): for traverse_iter the
    entries its own push rule asks for (room for both children is checked before either is pushed: the largest head + 2; rays
    from the far end, where the chain is the FAR child and piles up under the near leaves), for the recursive walk the pending
    right children.  Up to 128: distances bit-equal to the oracle's.  Beyond: the documented error and text, and the next call
    on the same context - a shallow mesh - is right (the flag word was reset)."""
    import torch
    (s_nodes, s_verts, s_idx), s_dev = _mesh_on_device(ctx, 12)
    s_rays, _, _ = chain_rays(700, 13.0, seed=9, near_x=-1.0)
    covered, outcome = [], []
    for n_tris in range(122, 142):
        (nodes, verts, idx), dev = _mesh_on_device(ctx, n_tris)
        rays, far_side, cheap = chain_rays(700, n_tris + 1.0, seed=n_tris, near_x=-1.0)
        if walk == "iter":
            want, need = oracle.traverse_iter(nodes, verts, idx, rays, depths=True)
            run = lambda dv, rr, out: ctx.traverse_iter_dev(*dv, ctx.upload(rr), len(rr), out)
            s_want = oracle.traverse_iter(s_nodes, s_verts, s_idx, s_rays)
            text = "vd_traverse_iter: traversal stack (128 entries per ray) exceeded"
        else:
            want, need = oracle.traverse_recursive(nodes, verts, idx, rays, depths=True)
            run = lambda dv, rr, out: ctx.traverse_dev(*dv, ctx.upload(rr), len(rr), out)
            s_want = oracle.traverse_recursive(s_nodes, s_verts, s_idx, s_rays)
            text = "vd_traverse: traversal stack (128 pending right children per ray) exceeded"
        top = int(need.max())
        hit = (want >= 0) & (want < np.float32(1e29))
        assert hit[need == top].sum() > 0, (n_tris, "every deepest ray misses")
        covered.append(top)
        d_out = torch.full((len(rays),), 7.0, dtype=torch.float32, device="cuda")
        if top <= 128:
            run(dev, rays, d_out)
            assert d_out.cpu().numpy().view(np.uint32).tobytes() == want.view(np.uint32).tobytes(), (walk, n_tris, top)
            outcome.append("ok")
        else:
            with pytest.raises(VoidinError) as e:
                run(dev, rays, d_out)
            assert e.value.code == abi.VD_ERR_STACK_OVERFLOW and text in str(e.value), (walk, n_tris, top, str(e.value))
            assert ctx.lib.vd_last_error(ctx.h).decode() == text
            outcome.append("overflow")
            d_s = torch.full((len(s_rays),), 7.0, dtype=torch.float32, device="cuda")
            run(s_dev, s_rays, d_s)
            assert d_s.cpu().numpy().view(np.uint32).tobytes() == s_want.view(np.uint32).tobytes(), (walk, n_tris, "the call after the error")
    print(f"\n{walk}: entries asked per length {covered} -> {outcome}")
    lo = covered[0]
    assert covered == list(range(lo, lo + len(covered))) and lo <= 120 and covered[-1] >= 136
    assert {127, 128, 129} <= set(covered)

