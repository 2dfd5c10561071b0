"""Scenes, depth buffers and ORACLE-side expected values for the occlusion-culled draw lists (vd_cull_compact_hiz*,
vd_cull_early_dev, vd_cull_late_dev).  Nothing here touches the GPU or the library under test: tests/test_cull_occlusion_abi.py
checks on the CPU that every case is non-vacuous, tests/test_gpu_cull_occlusion.py compares the GPU's bytes against what
these functions return.

    F = oracle.cull_emit(...).instance_count != 0          the frustum set
    V = oracle.occlusion_mask(..., F)                      F minus what the pyramid hides
    E = F & P,  L = V & ~P                                 early / late lists for visible-last-frame bits P
"""
import numpy as np

from voidin_amd import abi, synth

SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 8191, 8193, 200_000, (2 << 20) + 777]
PYRAMIDS = [(1, 1), (5, 3), (1920, 1080), (4097, 3)]
MESH_COUNTS = [16, 600, 66_000]                  # 1-, 2- and 4-byte ids
FULL_SIZE = 10_000_000
NON_VACUOUS_FROM = 5_000


def camera(frame=0):
    """The camera of tests/test_occlusion.py; frame > 0 moves and turns it (the three-frame loop)."""
    return synth.camera_uniform(eye=(4.0 * frame, -3.0 * frame, 50.0 + 6.0 * frame), yaw_deg=2.5 * frame, pitch_deg=-1.5 * frame,
                                jitter=(0.003, -0.002))


def meshes_for(n_mesh):
    meshes = synth.mesh_infos(n_mesh, seed=synth.SEED_BASE + (0 if n_mesh == 16 else 50))
    if n_mesh > 60_000:                          # base_index would overflow u32 with the default index counts
        meshes["index_count"] = 36
        meshes["base_index"] = np.arange(n_mesh, dtype=np.uint32) * 36
        meshes["vertex_offset"] = np.arange(n_mesh, dtype=np.int32) * 12
    return meshes


def cloud(n, seed=synth.SEED_BASE + 60, n_mesh=16):
    """tests/test_occlusion.py's _cloud, wider than the frustum (so |F| < n): in front of a camera at z = 50 looking down -z."""
    return synth.instances(n, n_mesh=n_mesh, seed=seed, extent=700.0, centre=(0.0, 0.0, -150.0), scale_range=(0.25, 4.0),
                           with_inverse=False)


def depth(w, h, seed=synth.SEED_BASE + 61):
    """tests/test_occlusion.py's _random_depth (rectangles of near occluders over a cleared background); buffers of a few
    texels get one occluder distance per texel instead, from the middle of the cloud's depth range."""
    if w * h < 64:
        u = synth.uniform01(seed, 1, w * h).reshape(h, w)
        return (0.001 / (120.0 + 200.0 * u)).astype(np.float32)
    u = synth.uniform01(seed, 0, 64 * 5).reshape(64, 5).astype(np.float64)
    d = np.zeros((h, w), dtype=np.float32)
    for x, y, sx, sy, z in u:
        x0, y0 = int(x * w), int(y * h)
        d[y0: y0 + 1 + int(sy * h / 3), x0: x0 + 1 + int(sx * w / 3)] = np.float32(0.001 / (20.0 + 300.0 * z))
    return d


def poisoned_cloud(n=4000):
    """The poisoned / near-plane cloud of tests/test_occlusion.py::test_gpu_occlusion_with_poisoned_and_near_plane_instances."""
    inst = synth.instances(n, seed=synth.SEED_BASE + 48, extent=300.0, centre=(0.0, 0.0, -150.0), scale_range=(0.25, 4.0))
    inst["transform"][10, 12] = np.nan
    inst["transform"][11, 0] = np.inf
    inst["transform"][12, :12] = 0.0                       # zero scale: radius 0
    inst["transform"][13, 14] = 50.0                       # at the eye
    inst["transform"][14, 14] = 500.0                      # far behind the camera
    inst["transform"][15:400, 14] = 50.0 - synth.uniform01(synth.SEED_BASE + 49, 0, 385).astype(np.float32) * 3.0   # straddling the near plane
    return inst


def bits(mask, n):
    return np.unpackbits(np.ascontiguousarray(mask).view(np.uint8), bitorder="little")[:n].astype(bool)


def pack(flags):
    """bool[n] -> ceil(n / 64) u64 words, padding bits 0."""
    n = len(flags)
    b = np.zeros(((n + 63) // 64) * 64, dtype=np.uint8)
    b[:n] = flags
    return np.packbits(b, bitorder="little").view(np.uint64).copy()


def random_prev(n, seed=synth.SEED_BASE + 62, set_padding=True):
    """Visible-last-frame words: about half the bits set; with set_padding the bits behind n are ALL ones (they must be ignored)."""
    words = (n + 63) // 64
    u = synth.uniform01(seed, 2, words * 4).reshape(words, 4)
    w = np.zeros(words, dtype=np.uint64)
    for k in range(4):
        w |= (u[:, k] * 65536.0).astype(np.uint64) << np.uint64(16 * k)
    if n % 64:
        pad = np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(n % 64)
        w[-1] = (w[-1] | pad) if set_padding else (w[-1] & ~pad)
    return w


def oracle_sets(oracle, cam, meshes, inst, pyramid, w, h, threads=8):
    """(draws of every instance, F, V) from the oracle alone."""
    n = len(inst)
    draws = oracle.cull_emit(cam, meshes, inst, threads=threads)
    F = draws["instance_count"] != 0
    V = bits(oracle.occlusion_mask(cam, meshes, inst, pyramid, w, h, pack(F)), n)
    return draws, F, V


def select(draws, flags):
    """The list the entry points write for the instances of `flags`: their rows of the oracle's emit_draws output (every one
    of them has instance_count == 1, because the lists are subsets of F)."""
    return np.ascontiguousarray(draws[np.flatnonzero(flags)])


def assert_not_vacuous(n, F, V, E=None, L=None):
    """A condition on the ORACLE's sets, checked before any GPU result is looked at."""
    assert not (V & ~F).any()
    if n < NON_VACUOUS_FROM:
        return
    f, v = int(F.sum()), int(V.sum())
    assert f < n, (n, f)
    assert v * 20 >= f, (n, f, v)                 # |V| >= 5 % of |F|
    assert (f - v) * 20 >= f, (n, f, v)           # |F \ V| >= 5 % of |F|
    if E is not None:
        assert int(E.sum()) > 0 and int(L.sum()) > 0, (n, int(E.sum()), int(L.sum()))
