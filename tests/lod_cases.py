"""Scenes, a numpy float32 TWIN of the level-of-detail definition (include/voidin_abi.h, "Level of detail") and the expected
draw lists of vd_cull_compact_lod* / vd_cull_batch_lod_dev / vd_lod_ids_dev.  Nothing here touches the GPU or loads the
library under test: tests/test_lod_cases.py checks on the CPU that every case is non-vacuous, tests/test_gpu_cull_lod.py
compares the GPU's bytes against what these functions return.

The twin restates the header's definition, one float32 operation per numpy call in the order written there (np.fmax where
the definition says fmaxf).  The expected lists take their frustum set from the ORACLE, not from the twin:

    draws = oracle.cull_emit(cam, base, inst),  base[g] = {G.min, G.max, ...}     F = draws.instance_count != 0
    drawn = F & ~(size < min_size)                                                 size, row: the twin's
    list  = {meshes[row[i]].index_count, 1, .base_index, .vertex_offset, i} for i in drawn, ascending
    batched form = that list stably sorted by row
"""
import numpy as np

import cull_occlusion_cases as K
from voidin_amd import abi, synth

SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 8191, 8193, 200_000]
STRIDE_SIZE = 3_300_077            # above 3 x 256 CUs x 4 waves x 1024 instances: pass 1's grid-stride loop is taken
ROW_COUNTS = [64, 600, 66_000]     # 1-, 2- and 4-byte ids
N_LODS = 4
NON_VACUOUS_FROM = 5_000
MIN_DISTANCE = np.float32(0.125)
f32 = np.float32

camera = K.camera


def params(cam, min_size=0.0):
    """size = the projected radius in pixels of a 1080-line viewport."""
    return {"scale": float(f32(540.0) * f32(cam["projection"].reshape(-1)[5])), "min_distance": float(MIN_DISTANCE),
            "min_size": float(f32(min_size))}


# --- the twin -------------------------------------------------------------------------------------------------------------
def _len3(x, y, z):
    return np.sqrt(((x * x) + (y * y)) + (z * z))


def twin(cam, P, groups, n_mesh, inst):
    """dict(size, lod, row, visible) per instance, float32 throughout."""
    with np.errstate(all="ignore"):
        cam = np.asarray(cam, dtype=abi.CAMERA).reshape(-1)[0]
        V = cam["view"].astype(f32)
        n_group = len(groups)
        G = groups[np.minimum(inst["mesh"], np.uint32(n_group - 1))]
        mn, mx = G["min"].astype(f32), G["max"].astype(f32)
        T = inst["transform"].astype(f32)
        col = [[T[:, 4 * j + k] for k in range(4)] for j in range(4)]      # col[j] = (x, y, z, w) of column j
        c0 = [(mx[:, a] + mn[:, a]) / f32(2.0) for a in range(3)]
        c = []
        for r in range(3):
            v = [V[4 * k + r] for k in range(4)]
            m = [(((v[0] * col[j][0]) + (v[1] * col[j][1])) + (v[2] * col[j][2])) + (v[3] * col[j][3]) for j in range(4)]
            c.append((((m[0] * c0[0]) + (m[1] * c0[1])) + (m[2] * c0[2])) + (m[3] * f32(1.0)))
        s = [np.abs(_len3(col[j][0], col[j][1], col[j][2])) for j in range(3)]
        max_scale = np.fmax(np.fmax(s[0], s[1]), s[2])
        # the frustum test (its radius is the reference's: object-space corners against the view-space centre)
        d0 = _len3(mn[:, 0] - c[0], mn[:, 1] - c[1], mn[:, 2] - c[2])
        d1 = _len3(mx[:, 0] - c[0], mx[:, 1] - c[1], mx[:, 2] - c[2])
        radius = np.fmax(d0, d1) * max_scale
        fr = cam["frustum"].astype(f32)
        out_x = ((c[2] * fr[1]) - (np.abs(c[0]) * fr[0])) < -radius
        out_y = ((c[2] * fr[3]) - (np.abs(c[1]) * fr[2])) < -radius
        out_z = ((c[2] + radius) > f32(cam["znear"])) & ((c[2] - radius) > f32(cam["zfar"]))
        visible = ~out_x & ~out_y & ~out_z
        # the size metric
        r = (_len3(mx[:, 0] - mn[:, 0], mx[:, 1] - mn[:, 1], mx[:, 2] - mn[:, 2]) * f32(0.5)) * max_scale
        d = -c[2]
        dist = np.fmax(d, f32(P["min_distance"]))
        size = (r * f32(P["scale"])) / dist
        nl = np.clip(G["n_lods"].astype(np.int64), 1, abi.LOD_MAX)
        lod = np.zeros(len(inst), dtype=np.int64)
        for k in range(abi.LOD_MAX - 1):
            lod += ((k < nl - 1) & (size < G["switch_size"][:, k].astype(f32))).astype(np.int64)
        first = np.minimum(G["first_row"].astype(np.int64), n_mesh - 1)
        row = np.minimum(first + lod, n_mesh - 1)
    return {"size": size.astype(f32), "lod": lod, "row": row, "visible": visible}


# --- scenes ---------------------------------------------------------------------------------------------------------------
def tables(n_rows, n_lods=N_LODS):
    """(base, meshes, groups): n_rows / n_lods groups whose boxes are base's, group g = rows [g n_lods, (g + 1) n_lods) of
    meshes; thresholds all 0 (every instance takes LOD 0) until with_thresholds sets them."""
    n_group = n_rows // n_lods
    base, meshes = K.meshes_for(n_group), K.meshes_for(n_rows)
    groups = np.zeros(n_group, dtype=abi.LOD_GROUP)
    groups["min"], groups["max"] = base["min"], base["max"]
    groups["first_row"] = np.arange(n_group, dtype=np.uint32) * n_lods
    groups["n_lods"] = n_lods
    return base, meshes, groups


def with_thresholds(groups, size_over_F, n_lods=N_LODS):
    """switch_size from the quantiles of the twin's size over the frustum set: every LOD takes an equal share."""
    g = groups.copy()
    if len(size_over_F):
        q = np.quantile(size_over_F.astype(np.float64), [1.0 - (k + 1) / n_lods for k in range(n_lods - 1)]).astype(f32)
        g["switch_size"][:, : n_lods - 1] = q
    return g


def commands(meshes, rows, idx):
    out = np.zeros(len(idx), dtype=abi.DRAW)
    m = meshes[rows]
    out["vertex_count"], out["instance_count"], out["base_index"] = m["index_count"], 1, m["base_index"]
    out["vertex_offset"], out["base_instance"] = m["vertex_offset"], idx
    return out


def expect(oracle, cam, P, base, meshes, groups, inst, threads=8):
    """dict(F, drawn, row, size, list, cmds, ids): the contract's outputs from the oracle's frustum set and the twin."""
    t = twin(cam, P, groups, len(meshes), inst)
    F = oracle.cull_emit(cam, base, inst, threads=threads)["instance_count"] != 0
    with np.errstate(invalid="ignore"):
        drawn = F & ~(t["size"] < f32(P["min_size"]))
    idx = np.flatnonzero(drawn)
    rows = t["row"][idx]
    order = np.argsort(rows, kind="stable")
    cnt = np.bincount(rows, minlength=len(meshes))
    cmds = np.zeros(len(meshes), dtype=abi.DRAW)
    cmds["vertex_count"], cmds["instance_count"], cmds["base_index"] = meshes["index_count"], cnt, meshes["base_index"]
    cmds["vertex_offset"], cmds["base_instance"] = meshes["vertex_offset"], np.cumsum(cnt) - cnt
    return {"F": F, "drawn": drawn, "row": t["row"], "size": t["size"], "lod": t["lod"], "visible": t["visible"],
            "list": commands(meshes, rows, idx.astype(np.uint32)), "cmds": cmds, "ids": idx[order].astype(np.uint32)}


def scene(oracle, n, n_rows=64, min_size_quantile=None, seed=synth.SEED_BASE + 60):
    """(cam, P, base, meshes, groups, inst): the occlusion cases' camera and cloud, thresholds at the quartiles of the size
    over the oracle's frustum set, min_size 0 or at that quantile of the same sizes."""
    cam = camera()
    base, meshes, groups = tables(n_rows)
    inst = K.cloud(n, seed=seed, n_mesh=len(groups))
    P = params(cam)
    t = twin(cam, P, groups, len(meshes), inst)
    F = oracle.cull_emit(cam, base, inst, threads=8)["instance_count"] != 0
    sizes = t["size"][F & np.isfinite(t["size"])]
    groups = with_thresholds(groups, sizes)
    if min_size_quantile is not None and len(sizes):
        P = params(cam, np.quantile(sizes.astype(np.float64), min_size_quantile).astype(f32))
    return cam, P, base, meshes, groups, inst


# --- hand-made instances --------------------------------------------------------------------------------------------------
HAND = ["eq_threshold", "eq_min_size", "nan", "inf", "zero_scale", "at_eye", "behind", "lods_1", "lods_8", "lods_0", "lods_9",
        "unsorted", "nan_box", "mesh_past_groups", "mesh_all_ones", "row_past_meshes", "first_row_all_ones"]
_UNSORTED = np.array([2.0, 0.5, 3.0, 0.25, 4.0, 0.125, 5.0], dtype=f32)       # four of the seven lie above 1


def hand_scene(oracle, n=3000):
    """A 64-row scene whose first len(HAND) instances inside the frustum become the hand-made cases, each with a group of
    its own behind the 16 ordinary ones; one more group, the last, is what instances beyond the table clamp to.  Returns
    (cam, P, base, meshes, groups, inst, where): where[name] = the instance index of the case."""
    cam, P, base, meshes, groups, inst = scene(oracle, n, 64, min_size_quantile=0.2)
    inst = inst.copy()
    n_rows = len(meshes)
    e = expect(oracle, cam, P, base, meshes, groups, inst)
    plain = np.flatnonzero(e["drawn"] & np.isfinite(e["size"]))[: len(HAND)]
    assert len(plain) == len(HAND)
    where = dict(zip(HAND, (int(i) for i in plain)))
    smallest = int(plain[np.argmin(e["size"][plain])])                  # min_size becomes ITS size: the other cases stay above
    for name in HAND:
        if where[name] == smallest:
            where[name], where["eq_min_size"] = where["eq_min_size"], smallest
            break
    own = {}                                       # case -> its group, a copy of the instance's ordinary one
    extra_g, extra_b = [], []
    for name in HAND:
        g0 = int(inst["mesh"][where[name]])
        own[name] = len(groups) + len(extra_g)
        extra_g.append(groups[g0].copy())
        extra_b.append(base[g0].copy())
    extra_g.append(groups[3].copy())               # the LAST group: what an instance beyond the table clamps to
    extra_b.append(base[3].copy())
    groups = np.concatenate([groups, np.array(extra_g, dtype=abi.LOD_GROUP)])
    base = np.concatenate([base, np.array(extra_b, dtype=abi.MESH_INFO)])
    for name in HAND:
        inst["mesh"][where[name]] = own[name]
    T = inst["transform"]
    T[where["nan"], 12] = np.nan
    T[where["inf"], 0] = np.inf
    T[where["zero_scale"], :12] = 0.0
    T[where["at_eye"], 12:15] = cam["view_position"].reshape(-1)[:3]
    T[where["behind"], 14] = 500.0
    inst["mesh"][where["mesh_past_groups"]] = len(groups) + 5
    inst["mesh"][where["mesh_all_ones"]] = 0xFFFFFFFF
    groups[-1]["first_row"] = 8
    size = twin(cam, P, groups, n_rows, inst)["size"]                   # thresholds play no part in it

    def g(name):
        return groups[own[name]]
    g("eq_threshold")["first_row"], g("eq_threshold")["n_lods"] = 4, 4
    g("eq_threshold")["switch_size"][:3] = [size[where["eq_threshold"]], 0.0, 0.0]      # strict <: stays on LOD 0
    P = dict(P, min_size=float(size[where["eq_min_size"]]))                             # strict <: is drawn
    for name, nl in (("lods_1", 1), ("lods_8", 8), ("lods_0", 0), ("lods_9", 9)):
        g(name)["first_row"], g(name)["n_lods"] = 20, nl
        g(name)["switch_size"][:] = np.inf                                              # every threshold that counts is above
    g("unsorted")["first_row"], g("unsorted")["n_lods"] = 30, 8
    g("unsorted")["switch_size"][:] = _UNSORTED * size[where["unsorted"]]
    g("nan_box")["first_row"], g("nan_box")["n_lods"] = 40, 4
    g("nan_box")["switch_size"][:] = np.inf                                             # a NaN size is below none of them
    g("nan_box")["max"][0] = np.nan
    base[own["nan_box"]]["max"][0] = np.nan
    g("row_past_meshes")["first_row"], g("row_past_meshes")["n_lods"] = n_rows - 2, 4
    g("row_past_meshes")["switch_size"][:] = np.inf
    g("first_row_all_ones")["first_row"], g("first_row_all_ones")["n_lods"] = 0xFFFFFFFF, 4
    g("first_row_all_ones")["switch_size"][:] = np.inf
    return cam, P, base, meshes, groups, inst, where
