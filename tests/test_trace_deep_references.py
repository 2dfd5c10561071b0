"""CPU half of tests/test_gpu_trace_deep.py: the C oracle that those tests hold the device against is itself held against the
second, independent restatement (oracle/np_restate.py: plain Python lists for stacks, no limit) at the depths where it is used
there - beyond the 256 entries its stacks had when the first deep tests were written."""
import numpy as np
import pytest

from chain_scenes import chain_blas_mesh, chain_blas_scene, chain_mixed_scene, chain_rays, chain_scene
from oracle import np_restate


@pytest.mark.parametrize("kind,length,n_rays", [("tlas", 1400, 110), ("blas", 1500, 90)])
def test_c_oracle_equals_numpy_restatement_at_depth(oracle, kind, length, n_rays):
    """Rays of the 4 Ki class (second iteration of the device's second pass) among shallow ones: `dist` bits, `hit` and the shared
    far-only depth of the two restatements agree."""
    scene = chain_scene(oracle, length) if kind == "tlas" else chain_blas_scene(oracle, length)
    rays, far_side, cheap = chain_rays(n_rays, length + 50.0, seed=7)
    want, deepest, depth = oracle.trace(scene, rays, depths=True)
    deep = depth > 1152
    assert deep.sum() >= 20 and want["hit"][deep].sum() > 0 and (depth <= 128).sum() >= 20
    got, got_depth = np_restate.trace(scene, rays, depths=True)
    assert got["dist"].view(np.uint32).tobytes() == want["dist"].view(np.uint32).tobytes()
    assert np.array_equal(got["hit"], want["hit"])
    assert np.array_equal(got_depth, depth)


def test_depth_outputs_change_nothing_else(oracle):
    """oracle.trace with and without the depth outputs: same records, same deepest stack use; the far-only depth is never above
    it (it leaves the near child out); a ray that hits nothing has no first-hit depth, one that hits has one within its depth."""
    scene = chain_mixed_scene(oracle, 300, 200)
    rays, far_side, cheap = chain_rays(1500, 350.0, seed=3)
    plain, deepest = oracle.trace(scene, rays, threads=4)
    want, deepest2, depth, at_hit = oracle.trace(scene, rays, threads=4, first_hit=True)
    assert plain.tobytes() == want.tobytes() and deepest == deepest2
    assert depth.max() == 300 + 200 - 4 and depth.max() <= 2 * deepest
    assert np.array_equal(at_hit == 0xFFFFFFFF, want["hit"] == 0)
    assert (at_hit[want["hit"] == 1] <= depth[want["hit"] == 1]).all()
    small = chain_mixed_scene(oracle, 12, 9)
    r2 = rays[:40].copy(); r2["eye"][r2["eye"][:, 0] > 0, 0] = np.float32(60.0)
    w2, _, d2 = oracle.trace(small, r2, depths=True)
    g2, gd2 = np_restate.trace(small, r2, depths=True)
    assert g2["dist"].view(np.uint32).tobytes() == w2["dist"].view(np.uint32).tobytes() and np.array_equal(gd2, d2)


def test_traverse_depth_outputs(oracle):
    """The BLAS-only walks: distances unchanged by asking for depths, and the depths of the chain mesh are the ones its
    construction gives - n - 3 interior levels: the recursive walk holds one pending right child per level; traverse_iter, for
    a ray from the far end (the chain is its far child at every level), one near leaf per level plus the pair it is about to push."""
    for n in (40, 300):
        nodes, verts, idx = chain_blas_mesh(n)
        rays, far_side, cheap = chain_rays(300, n + 1.0, seed=n, near_x=-1.0)
        d, need = oracle.traverse_iter(nodes, verts, idx, rays, depths=True)
        assert d.tobytes() == oracle.traverse_iter(nodes, verts, idx, rays).tobytes()
        assert need[far_side & ~cheap].max() == need.max() == (n - 3) + 1 and need[~far_side & ~cheap].max() == 2
        r, pend = oracle.traverse_recursive(nodes, verts, idx, rays, depths=True)
        assert r.tobytes() == oracle.traverse_recursive(nodes, verts, idx, rays).tobytes()
        assert pend[~cheap].max() == n - 3 and (pend[cheap] == 0).all()
