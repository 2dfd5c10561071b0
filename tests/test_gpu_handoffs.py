"""Run-time half of the hand-offs between workgroups inside ONE launch ("In-launch hand-offs"): a box, a count word
or a ticket written by one workgroup and read by another with nothing but write-through stores, a drained wave and a relaxed
agent-scope atomic in between (or two fences).  A kernel that gets this wrong reads a STALE word - and a stale word is invisible
as long as every launch is handed the input of the launch before: the old bytes are the right bytes.

ONE table-driven test.  A case names the kernels it exercises (tests/test_isa_protocols.py requires every kernel with a global
atomic or an agent-scope access to be covered here, in tests/test_gpu_stress.py, or excused with a reason), uploads the inputs of
tests/handoff_cases.py and their expected outputs ONCE, and then runs the entry point K times on the same buffers and the same
context, cycling A, B1, (B2), A, ... so that every word that changes hands differs from what the launch before left there
(tests/test_handoff_cases.py proves that on the CPU).  After each launch the output is compared ON THE DEVICE with the uploaded
expectation; only the verdict comes back.  A mismatch is a failure that names the launch, the input and the first differing node.

Two modes, because a stale read needs the wrong timing and placement to show: uniform and uneven load.  Quiet: nothing else runs.  Busy: a second
context on its own stream gets ten vd_cull_compact_dev calls over 3 000 001 instances enqueued before every ten launches and is
not waited for until the end - other workgroups on the CUs, other traffic through the L2s; nothing waits on it.

No case waits on a flag, changes an option that makes a kernel spin, or touches a byte outside its buffers.

Sensitivity, recorded once on an MI355X with a library whose leaf_climb (blas_refit.hip) read the sibling's six box words with
plain loads after a plain read of the same line before the counter add (links, indices and counters untouched): of the three
fence-free refit cases one turned red - blas_refit[three-fences0]-busy, launch 42, input A, nine node fields holding the boxes of
the launch before - the two quiet ones and the fenced ones (whose acquire invalidates the L1) stayed green, and so did
refit(build(x), x) == build(x) on all eight fixtures.  The alternation can see a stale box, where the identity cannot; it does not
see every one (one run of each case: no rate is claimed)."""
import numpy as np
import pytest

import handoff_cases as H
from conftest import first_difference
from test_gpu_tlas_lbvh import _check_structure
from voidin_amd import abi, synth
from voidin_amd.runtime import VoidinError

pytestmark = pytest.mark.gpu

K_CLIMB = 200        # launches of a single-launch climb: what tests/test_gpu_stress.py gives a climb
K_BUILD = 20         # alternations of vd_bvh_build_dev: each is hundreds of dependent launches (the stress file's build loops: 4 to 6)
N_MESH = 16

CASES = {}           # case id -> (function, parameter, kernels)


def case(*kernels, params):
    """params: [(id suffix, parameter, also run with the busy neighbour)]"""
    def deco(fn):
        for suffix, p, busy in params:
            for mode in ("quiet", "busy") if busy else ("quiet",):
                CASES[f"{fn.__name__}[{suffix}]-{mode}"] = (fn, p, kernels)
        return fn
    return deco


class Neighbour:
    """The busy neighbour: its own context, its own stream, its own buffers."""
    N = 3_000_001

    def __init__(self):
        import torch
        from voidin_amd.runtime import Context
        self.stream = torch.cuda.Stream()
        self.ctx = Context(0, use_torch_stream=False)
        self.ctx.set_stream(self.stream.cuda_stream)
        self.cam, meshes = synth.camera_uniform(), synth.mesh_infos()
        self.d_m = self.ctx.upload(meshes)
        self.d_i = self.ctx.upload(synth.instances(self.N, seed=synth.SEED_BASE + 3, with_inverse=False))
        self.d_o, self.d_c = self.ctx.empty(self.N * 20), torch.zeros(4, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        self.burst()
        self.stream.synchronize()
        self.count = int(self.d_c[0].item())
        assert 0 < self.count < self.N

    def burst(self):
        for _ in range(10):
            self.ctx.cull_compact_dev(self.cam, self.d_m, N_MESH, self.d_i, self.N, self.d_o, self.d_c)

    def finish(self):
        self.stream.synchronize()
        assert int(self.d_c[0].item()) == self.count, "the neighbour's own list changed"

    def close(self):
        self.stream.synchronize()
        self.ctx.close()


@pytest.fixture(scope="module")
def neighbour():
    made = []

    def get():
        if not made:
            made.append(Neighbour())
        return made[0]
    yield get
    for nb in made:
        nb.close()


class Env:
    def __init__(self, ctx, oracle, ctx_options, neighbour):
        self.ctx, self.oracle, self.opt, self.neighbour = ctx, oracle, ctx_options, neighbour

    def alternate(self, K, tags, launch, verdict, explain):
        """launch(j) stages input j and enqueues the entry point; verdict(j) -> bool, computed on the device; explain(j) -> what
        differs, computed on the host and only after a mismatch."""
        nb = self.neighbour
        for k in range(K):
            j = k % len(tags)
            if nb is not None and k % 10 == 0:
                nb.burst()
            try:
                launch(j)
                ok = verdict(j)
            except VoidinError as err:
                if err.code == abi.VD_ERR_HIP:             # the device may have faulted: start nothing more on it
                    pytest.exit(f"launch {k}, input {tags[j]}: {err}", returncode=3)
                raise
            if not ok:
                pytest.fail(f"launch {k}, input {tags[j]}: {explain(j)}")
        if nb is not None:
            nb.finish()


def _bytes_differ(got, want, what):
    a, b = np.frombuffer(got.cpu().numpy().tobytes(), np.uint8), np.frombuffer(want.cpu().numpy().tobytes(), np.uint8)
    d = np.flatnonzero(a != b)
    return f"{what}: equal" if not d.size else f"{what}: first difference at byte {int(d[0])} (word {int(d[0]) // 4}), {d.size} bytes differ"


def _nodes_differ(got, want, dtype, what):
    g, w = got.cpu().numpy().view(dtype), want.cpu().numpy().view(dtype)
    d = first_difference(g, w)
    if d is None:
        return f"{what}: equal"
    wrong = int(sum((np.ascontiguousarray(g[f]).view(np.uint32).reshape(len(g), -1) != np.ascontiguousarray(w[f]).view(np.uint32).reshape(len(w), -1)).any(axis=1).sum()
                    for f in g.dtype.names))
    return f"{what}: first differing node {d[1]} (field {d[0]}: got {g[d[0]][d[1]]}, want {w[d[0]][d[1]]}); {wrong} node fields differ"


def _assert_teeth(a, b, interior, what):
    holds, kept = H.teeth(a, b, interior)
    assert holds, f"{what}: {kept} interior nodes keep their box between the inputs - the alternation would not see them stale"


# ---- vd_tlas_refit[_wide]_dev: the climb of tlas_refit_up_kernel --------------------------------------------------------------------

@case("tlas_refit_up_kernel", params=[("narrow-4096", (4096, False), True), ("narrow-32768", (32768, False), False), ("wide-40000", (40000, True), True)])
def tlas_refit(e, p):
    """ONE topology - the LBVH top level of A, renumbered children-first - refitted for A and for the moved instances in turn:
    every byte of the node array == oracle.tlas_refit of that instance set over that topology."""
    import torch
    n, wide = p
    ctx, dt = e.ctx, abi.TLAS_NODE_WIDE if wide else abi.TLAS_NODE
    meshes, inputs = H.tlas_refit_inputs(n)
    d_m, d_in = ctx.upload(meshes), [ctx.upload(inst) for _, inst in inputs]
    d_i, d_t = d_in[0].clone(), ctx.empty((2 * n + 1) * dt.itemsize)
    ctx.tlas_build_lbvh_dev(d_i, n, d_m, N_MESH, d_t, wide=wide)
    torch.cuda.synchronize()
    topology = H.children_first(d_t.cpu().numpy().view(dt))
    want = H.tlas_refit_expected(e.oracle, topology, meshes, inputs)
    _assert_teeth(want[0], want[1], H.tlas_interior(want[0]), f"n = {n}")
    d_t.copy_(ctx.upload(topology))
    d_want = [ctx.upload(w) for w in want]

    def launch(j):
        d_i.copy_(d_in[j])
        ctx.tlas_refit_dev(d_i, n, d_m, N_MESH, d_t, wide=wide)

    e.alternate(K_CLIMB, [t for t, _ in inputs], launch, lambda j: torch.equal(d_t, d_want[j]),
                lambda j: _nodes_differ(d_t, d_want[j], dt, "top-level nodes"))


# ---- vd_bvh_refit_planned_dev: the leaf climb and the MeshInfo fold of blas_refit_kernel<fences> -----------------------------------

@case("blas_refit_kernel", params=[(f"{plan}-fences{f}", (plan, f), plan == "three") for plan in H.REFIT_PLANS for f in (0, 1)])
def blas_refit(e, p):
    """One plan over meshes packed into ONE node, vertex and MeshInfo buffer: min / max of every node == refit_reference, every
    other field as uploaded; MeshInfo.min / max == mesh_bounds_reference, its other 24 bytes zero as uploaded."""
    import torch
    plan_name, fences = p
    ctx = e.ctx
    e.opt("blas.refit_fences", fences)
    built, inputs = H.blas_refit_inputs(plan_name, e.oracle)
    M = len(built)
    v_off = np.concatenate([[0], np.cumsum([len(v) for v, _, _ in built])])
    n_off = np.concatenate([[0], np.cumsum([len(nd) for _, _, nd in built])])
    d_idx = [ctx.upload(idx) for _, idx, _ in built]
    d_vin, d_want_n, d_want_i = [], [], []
    for tag, verts in inputs:
        want = H.blas_refit_expected(built, verts)
        info = np.zeros(M, dtype=abi.MESH_INFO)
        for m, (_, (lo, hi)) in enumerate(want):
            info["min"][m], info["max"][m] = lo, hi
        d_vin.append(ctx.upload(np.concatenate([np.ascontiguousarray(v, dtype=np.float32) for v in verts])))
        d_want_n.append(ctx.upload(np.concatenate([nd for nd, _ in want])))
        d_want_i.append(ctx.upload(info))
    host_a = d_want_n[0].cpu().numpy().view(abi.BVH_NODE)
    _assert_teeth(host_a, d_want_n[1].cpu().numpy().view(abi.BVH_NODE), np.concatenate([H.blas_interior(nd) for _, _, nd in built]), plan_name)
    d_v, d_n = d_vin[0].clone(), ctx.upload(np.concatenate([nd for _, _, nd in built]))
    d_info = ctx.upload(np.zeros(M, dtype=abi.MESH_INFO))
    items = (abi.BvhRefitItem * M)()
    for m, (v, idx, nd) in enumerate(built):
        items[m].verts_xyz, items[m].indices = abi.ptr(d_v) + 12 * int(v_off[m]), abi.ptr(d_idx[m])
        items[m].nodes, items[m].mesh_info = abi.ptr(d_n) + 32 * int(n_off[m]), abi.ptr(d_info) + 48 * m
        items[m].n_vert, items[m].n_tri, items[m].n_nodes = len(v), len(idx) // 3, len(nd)
    plan = ctx.bvh_refit_plan(items)
    try:
        assert all(items[m].status == 0 for m in range(M))

        def launch(j):
            d_v.copy_(d_vin[j])
            ctx.bvh_refit_planned(plan)

        e.alternate(K_CLIMB, [t for t, _ in inputs], launch, lambda j: torch.equal(d_n, d_want_n[j]) and torch.equal(d_info, d_want_i[j]),
                    lambda j: _nodes_differ(d_n, d_want_n[j], abi.BVH_NODE, f"nodes (meshes start at {n_off[:-1].tolist()})") + "; " +
                    _bytes_differ(d_info, d_want_i[j], "MeshInfo"))
    finally:
        plan.close()


# ---- vd_bvh_build_lbvh_dev: fit_body of blas_lbvh_fit_kernel (boxes and the count / height word) ---------------------------------

@case("blas_lbvh_fit_kernel", params=[("soup4097", ("soup4097", 0), True), ("soup4097-depth12", ("soup4097", 12), True), ("helmet", ("helmet", 0), False)])
def blas_lbvh(e, p):
    """[0, n_nodes) of the nodes, the permuted indices and the result record == lbvh_reference / lbvh_bounded_reference of that
    input.  (VD_OPT_BLAS_LBVH_MAX_DEPTH = 12 is refused for the helmet's 15 452 triangles: tests/test_handoff_cases.py.)"""
    import torch
    name, bound = p
    ctx = e.ctx
    if bound:
        e.opt("blas.lbvh_max_depth", bound)
    inputs, want = H.lbvh_inputs(name), H.lbvh_expected(name, bound)
    n_vert, T = len(inputs[0][1]), len(inputs[0][2]) // 3
    cap = max(2, 2 * T)
    _assert_teeth(want[0]["nodes"], want[1]["nodes"], H.blas_interior(want[0]["nodes"]), name)
    assert H.meta_teeth(want[0]["nodes"], want[2]["nodes"]) >= 0.5
    d_vin = [ctx.upload(np.ascontiguousarray(v, dtype=np.float32)) for _, v, _ in inputs]
    d_iin = [ctx.upload(np.ascontiguousarray(i, dtype=np.uint32)) for _, _, i in inputs]
    d_v, d_i = d_vin[0].clone(), d_iin[0].clone()
    d_n = torch.full((cap * 32,), 0xCD, dtype=torch.uint8, device="cuda")
    d_r = torch.full((16,), 0xEE, dtype=torch.uint8, device="cuda")
    d_want_n = [ctx.upload(w["nodes"]) for w in want]
    d_want_i = [ctx.upload(w["indices"]) for w in want]
    d_want_r = [ctx.upload(np.array([(w["n_nodes"], w["n_bad_indices"], w["max_depth"], 0)], dtype=abi.BVH_LBVH_RESULT)) for w in want]
    nb = [32 * w["n_nodes"] for w in want]
    assert all(b <= cap * 32 for b in nb) and all(len(x) == len(d_v) for x in d_vin) and all(len(x) == len(d_i) == 12 * T for x in d_iin)

    def launch(j):
        d_v.copy_(d_vin[j]); d_i.copy_(d_iin[j])              # the build permutes the indices in place
        ctx.bvh_build_lbvh_dev(d_v, n_vert, d_i, T, d_n, cap, d_r)

    def explain(j):
        return "; ".join([_bytes_differ(d_r, d_want_r[j], "result record"), _nodes_differ(d_n[: nb[j]], d_want_n[j], abi.BVH_NODE, "nodes"),
                          _bytes_differ(d_i, d_want_i[j], "indices")])

    e.alternate(K_CLIMB, [t for t, _, _ in inputs], launch,
                lambda j: torch.equal(d_r, d_want_r[j]) and torch.equal(d_n[: nb[j]], d_want_n[j]) and torch.equal(d_i, d_want_i[j]), explain)


# ---- vd_bvh_build_lbvh_planned_dev: blas_lbvh_batch_fit_kernel, and the MeshInfo fold of blas_lbvh_batch_bounds_kernel -------------

@case("blas_lbvh_batch_fit_kernel", "blas_lbvh_batch_bounds_kernel", params=[("caps-3-4-300-1025-4097", None, True)])
def blas_lbvh_planned(e, p):
    """Five meshes under one plan; the vertices AND the count vector in device memory alternate.  Each mesh == the restatement of
    the single build of its first min(count, cap) triangles: result record, [0, n_nodes) of its nodes, its whole index buffer (the
    first 3 T permuted, the rest as put there); a count of 0 writes a zero record and nothing else; MeshInfo.min / max ==
    mesh_bounds_reference over all its vertices."""
    import torch
    ctx, caps = e.ctx, H.PLAN_CAPS
    inp, want = H.lbvh_plan_inputs(), H.lbvh_plan_expected()
    tags, M = list(inp), len(caps)
    d_vin = {t: [ctx.upload(np.ascontiguousarray(v, dtype=np.float32)) for v in inp[t][0]] for t in tags}
    d_iin = {t: [ctx.upload(np.ascontiguousarray(i, dtype=np.uint32)) for i in inp[t][1]] for t in tags}
    d_cin = {t: torch.from_numpy(np.asarray(inp[t][2], dtype=np.uint32).view(np.int32)).cuda() for t in tags}
    d_v, d_i = [x.clone() for x in d_vin["A"]], [x.clone() for x in d_iin["A"]]
    d_n = [torch.full((32 * max(2, 2 * c),), 0xCD, dtype=torch.uint8, device="cuda") for c in caps]
    d_res = torch.full((16 * M,), 0xEE, dtype=torch.uint8, device="cuda")
    d_cnt, d_info = d_cin["A"].clone(), ctx.upload(np.zeros(M, dtype=abi.MESH_INFO))
    items = (abi.BvhLbvhBatchItem * M)()
    for m, cap in enumerate(caps):
        n_vert = len(inp["A"][0][m])
        assert all(len(inp[t][0][m]) == n_vert and len(inp[t][1][m]) == 3 * cap for t in tags)
        items[m].verts_xyz, items[m].indices_inout, items[m].nodes = abi.ptr(d_v[m]), abi.ptr(d_i[m]), abi.ptr(d_n[m])
        items[m].mesh_info = abi.ptr(d_info) + 48 * m
        items[m].n_vert, items[m].tri_cap, items[m].node_cap = n_vert, cap, max(2, 2 * cap)
    d_want = {}
    for t in tags:
        res, info, per_mesh = np.zeros(M, dtype=abi.BVH_LBVH_RESULT), np.zeros(M, dtype=abi.MESH_INFO), []
        for m, w in enumerate(want[t]):
            info["min"][m], info["max"][m] = H.mesh_bounds_reference(inp[t][0][m])
            idx = np.array(inp[t][1][m], dtype=np.uint32, copy=True)
            if w is None:
                per_mesh.append((0, None, ctx.upload(idx)))
                continue
            res[m] = (w["n_nodes"], w["n_bad_indices"], w["max_depth"], 0)
            idx[: len(w["indices"])] = w["indices"]
            per_mesh.append((32 * w["n_nodes"], ctx.upload(w["nodes"]), ctx.upload(idx)))
        d_want[t] = (ctx.upload(res), ctx.upload(info), per_mesh)
    k = caps.index(1025)
    _assert_teeth(want["A"][k]["nodes"], want["B1"][k]["nodes"], H.blas_interior(want["A"][k]["nodes"]), "the 1025-triangle mesh")
    plan = ctx.bvh_lbvh_plan(items)
    try:
        assert all(it.status == 0 for it in items)

        def launch(j):
            t = tags[j]
            for m in range(M):
                d_v[m].copy_(d_vin[t][m]); d_i[m].copy_(d_iin[t][m])
            d_cnt.copy_(d_cin[t])
            ctx.bvh_build_lbvh_planned_dev(plan, d_cnt, d_res)

        def verdict(j):
            res, info, per_mesh = d_want[tags[j]]
            return (torch.equal(d_res, res) and torch.equal(d_info, info) and
                    all(torch.equal(d_i[m], idx) and (nodes is None or torch.equal(d_n[m][:nb], nodes)) for m, (nb, nodes, idx) in enumerate(per_mesh)))

        def explain(j):
            res, info, per_mesh = d_want[tags[j]]
            out = [_bytes_differ(d_res, res, "result records"), _bytes_differ(d_info, info, "MeshInfo")]
            for m, (nb, nodes, idx) in enumerate(per_mesh):
                if nodes is not None and not torch.equal(d_n[m][:nb], nodes):
                    out.append(_nodes_differ(d_n[m][:nb], nodes, abi.BVH_NODE, f"mesh {m} nodes"))
                if not torch.equal(d_i[m], idx):
                    out.append(_bytes_differ(d_i[m], idx, f"mesh {m} indices"))
            return "; ".join(out)

        e.alternate(K_CLIMB, tags, launch, verdict, explain)
    finally:
        plan.close()


# ---- vd_tlas_build_lbvh[_wide]_dev: lbvh_fit_kernel<VdTlasNode / VdTlasNodeWide>, the __threadfence() form --------------------------

_ACCEPTED = {}


@case("lbvh_fit_kernel", params=[("narrow-4096", (4096, False), True), ("wide-40000", (40000, True), True)])
def tlas_lbvh(e, p):
    """No byte-level restatement exists for the LBVH top level: for each input, the array tests/test_gpu_tlas_lbvh.py::_check_structure
    has accepted (layout, code order, FRESH bottom-up unions) is the expectation, and every launch of that input must equal it."""
    import torch
    n, wide = p
    ctx, dt = e.ctx, abi.TLAS_NODE_WIDE if wide else abi.TLAS_NODE
    meshes, inputs = H.tlas_lbvh_inputs(n)
    if p not in _ACCEPTED:                                    # computed once, shared by the two modes, never written
        _ACCEPTED[p] = [_check_structure(ctx, inst, meshes, wide) for _, inst in inputs]
    d_m, d_in, d_want, host = ctx.upload(meshes), [], [], []
    for nodes, d_inst, _, d_nodes in _ACCEPTED[p]:
        d_in.append(d_inst); d_want.append(d_nodes); host.append(nodes)
    for x, y in ((0, 1), (1, 2), (2, 0)):
        _assert_teeth(host[x], host[y], H.tlas_interior(host[x]), f"{inputs[x][0]} / {inputs[y][0]}")
    d_i, d_t = d_in[0].clone(), torch.full_like(d_want[0], 0x11)

    def launch(j):
        d_i.copy_(d_in[j])
        ctx.tlas_build_lbvh_dev(d_i, n, d_m, N_MESH, d_t, wide=wide)

    e.alternate(K_CLIMB, [t for t, _ in inputs], launch, lambda j: torch.equal(d_t, d_want[j]),
                lambda j: _nodes_differ(d_t, d_want[j], dt, "top-level nodes"))


# ---- vd_bvh_build_dev: the phase-A controls of blas.hip (the ctl->arrived ticket of a_boundary_kernel, the cnt_next adds) -----------

@case("a_boundary_kernel", "a_apply_kernel", params=[("soup3000", "soup3000", False), ("soup9000", "soup9000", True), ("knot32k", "knot32k", False)])
def bvh_build(e, name):
    """n_nodes, [0, n_nodes) of the nodes and the permuted indices == oracle.bvh_build of that input."""
    import torch
    ctx = e.ctx
    inputs, want = H.bvh_build_inputs(name), H.bvh_build_expected(e.oracle, name)
    n_vert, T = len(inputs[0][1]), len(inputs[0][2]) // 3
    cap = max(2, 2 * T)
    assert len(want[0][0]) == len(want[1][0])
    _assert_teeth(want[0][0], want[1][0], H.blas_interior(want[0][0]), name)
    assert H.meta_teeth(want[0][0], want[2][0]) >= 0.5
    d_vin = [ctx.upload(np.ascontiguousarray(v, dtype=np.float32)) for _, v, _ in inputs]
    d_iin = [ctx.upload(np.ascontiguousarray(i, dtype=np.uint32)) for _, _, i in inputs]
    d_v, d_i = d_vin[0].clone(), d_iin[0].clone()
    d_n = torch.full((cap * 32,), 0xCD, dtype=torch.uint8, device="cuda")
    d_want_n, d_want_i = [ctx.upload(nd) for nd, _ in want], [ctx.upload(idx) for _, idx in want]
    got_n = [0]
    assert all(len(nd) <= cap for nd, _ in want) and all(len(x) == len(d_v) for x in d_vin) and all(len(x) == len(d_i) == 12 * T for x in d_iin)

    def launch(j):
        d_v.copy_(d_vin[j]); d_i.copy_(d_iin[j])              # the build permutes the indices in place
        got_n[0] = ctx.bvh_build_dev(d_v, n_vert, d_i, T, d_n, cap)

    def explain(j):
        nb = 32 * min(got_n[0], len(want[j][0]))
        return "; ".join([f"n_nodes {got_n[0]}, want {len(want[j][0])}", _nodes_differ(d_n[:nb], d_want_n[j][:nb], abi.BVH_NODE, "nodes"),
                          _bytes_differ(d_i, d_want_i[j], "indices")])

    e.alternate(K_BUILD * len(inputs), [t for t, _, _ in inputs], launch,
                lambda j: got_n[0] == len(want[j][0]) and torch.equal(d_n[: 32 * got_n[0]], d_want_n[j]) and torch.equal(d_i, d_want_i[j]), explain)


@pytest.mark.parametrize("case_id", list(CASES))
def test_handoff(ctx, oracle, ctx_options, neighbour, case_id):
    fn, param, _ = CASES[case_id]
    fn(Env(ctx, oracle, ctx_options, neighbour() if case_id.endswith("-busy") else None), param)
