"""tests/lod_cases.py on the CPU, before any GPU result exists: the scenes populate every level of detail, contribution
culling drops a real share, the hand-made instances land where they were aimed, and the twin's own restatement of the
frustum test agrees with the oracle's."""
import functools

import numpy as np
import pytest

import lod_cases as L


@functools.lru_cache(maxsize=None)
def case(oracle_mod, n, n_rows, q):
    cam, P, base, meshes, groups, inst = L.scene(oracle_mod, n, n_rows, q)
    return P, groups, inst, L.expect(oracle_mod, cam, P, base, meshes, groups, inst)


@pytest.mark.parametrize("n_rows", L.ROW_COUNTS)
@pytest.mark.parametrize("n", [n for n in L.SIZES if n >= L.NON_VACUOUS_FROM])
def test_every_lod_is_populated(oracle, n, n_rows):
    P, groups, inst, e = case(oracle, n, n_rows, None)
    f = int(e["F"].sum())
    assert 0 < f < n
    share = np.bincount(e["lod"][e["F"]], minlength=L.N_LODS) / f
    print(n, n_rows, f, share)
    assert len(share) == L.N_LODS and (share >= 0.05).all(), share
    assert (e["row"] == groups["first_row"][inst["mesh"]] + e["lod"]).all()
    assert e["drawn"].tobytes() == e["F"].tobytes()                      # min_size = 0: off


@pytest.mark.parametrize("n", [n for n in L.SIZES if n >= L.NON_VACUOUS_FROM])
def test_contribution_culling_drops_a_fifth(oracle, n):
    P, groups, inst, e = case(oracle, n, 64, 0.2)
    f, d = int(e["F"].sum()), int(e["drawn"].sum())
    print(n, f, d, P)
    assert P["min_size"] > 0 and 0.10 * f <= f - d <= 0.30 * f, (f, d)
    assert not (e["drawn"] & ~e["F"]).any()


@pytest.mark.parametrize("n", L.SIZES)
def test_the_twins_frustum_test_is_the_oracles(oracle, n):
    P, groups, inst, e = case(oracle, n, 64, None)
    assert e["visible"].tobytes() == e["F"].tobytes()


def test_the_cloud_reaches_behind_the_camera(oracle):
    """... so the min_distance clamp decides sizes inside the frustum set, not only outside it."""
    cam, P, base, meshes, groups, inst = L.scene(oracle, 200_000, 64)
    e = L.expect(oracle, cam, P, base, meshes, groups, inst)
    far = L.twin(cam, dict(P, min_distance=1e-6), groups, len(meshes), inst)["size"]
    with np.errstate(invalid="ignore"):
        clamped = e["F"] & (far != e["size"])
    print(int(clamped.sum()), "sizes of the frustum set are decided by min_distance")
    assert clamped.sum() > 0


def test_hand_made_instances_land_where_intended(oracle):
    cam, P, base, meshes, groups, inst, where = L.hand_scene(oracle)
    n_rows = len(meshes)
    e = L.expect(oracle, cam, P, base, meshes, groups, inst)
    assert sorted(where) == sorted(L.HAND) and len(set(where.values())) == len(L.HAND)
    assert e["visible"].tobytes() == e["F"].tobytes()
    size, lod, row, drawn = e["size"], e["lod"], e["row"], e["drawn"]
    i = where["eq_threshold"]
    g = groups[inst["mesh"][i]]
    assert size[i] == g["switch_size"][0] and lod[i] == 0 and row[i] == 4 and drawn[i]
    up = groups.copy()
    up["switch_size"][inst["mesh"][i], 0] = np.nextafter(size[i], np.float32(np.inf))
    assert L.twin(cam, P, up, n_rows, inst)["lod"][i] == 1               # one ulp more and it switches
    i = where["eq_min_size"]
    assert size[i] == np.float32(P["min_size"]) and drawn[i]
    assert not L.expect(oracle, cam, dict(P, min_size=float(np.nextafter(size[i], np.float32(np.inf)))), base, meshes, groups, inst)["drawn"][i]
    assert 0.05 * e["F"].sum() <= e["F"].sum() - drawn.sum()              # that min_size drops a real share of the scene
    i = where["nan"]
    assert np.isfinite(size[i]) and size[i] > 1e3 and lod[i] == 0        # a NaN depth: dist = min_distance
    assert np.isinf(size[where["inf"]]) and lod[where["inf"]] == 0
    i = where["zero_scale"]
    assert size[i] == 0 and lod[i] == 3 and not drawn[i]
    for name in ("at_eye", "behind"):                                    # dist = min_distance: a huge size, the finest level
        assert size[where[name]] > 1e3 and lod[where[name]] == 0, name
    assert (lod[where["lods_1"]], row[where["lods_1"]]) == (0, 20)
    assert (lod[where["lods_0"]], row[where["lods_0"]]) == (0, 20)        # clamped to 1
    assert (lod[where["lods_8"]], row[where["lods_8"]]) == (7, 27)
    assert (lod[where["lods_9"]], row[where["lods_9"]]) == (7, 27)        # clamped to 8
    assert (lod[where["unsorted"]], row[where["unsorted"]]) == (4, 34)    # a count: 2, 3, 4 and 5 times the size lie above it
    i = where["nan_box"]
    assert np.isnan(size[i]) and (lod[i], row[i]) == (0, 40)
    last = len(groups) - 1
    for name in ("mesh_past_groups", "mesh_all_ones"):
        i = where[name]
        assert inst["mesh"][i] > last and 8 <= row[i] < 12 and drawn[i], name
        assert row[i] == 8 + lod[i]
    assert row[where["row_past_meshes"]] == n_rows - 1 and lod[where["row_past_meshes"]] == 3
    assert row[where["first_row_all_ones"]] == n_rows - 1
    in_list = [name for name in L.HAND if drawn[where[name]]]           # the cases the GPU's LIST shows; vd_lod_ids_dev shows all
    print("drawn:", in_list)
    assert set(L.HAND) - set(in_list) <= {"zero_scale", "nan_box"}


def test_synth_lod_groups_builds_rows_and_groups(oracle):
    from voidin_amd import abi, synth
    meshes = synth.mesh_infos(16)
    rows, groups = synth.lod_groups(meshes, 4, switch_size=(50.0, 12.0, 3.0))
    assert len(rows) == 64 and len(groups) == 16 and rows.dtype == abi.MESH_INFO and groups.dtype == abi.LOD_GROUP
    assert (groups["first_row"] == np.arange(16) * 4).all() and (groups["n_lods"] == 4).all()
    assert groups["min"].tobytes() == meshes["min"].tobytes() and groups["max"].tobytes() == meshes["max"].tobytes()
    assert (groups["switch_size"][:, :3] == [50.0, 12.0, 3.0]).all() and (groups["switch_size"][:, 3:] == 0).all()
    assert (rows["index_count"][0::4] == meshes["index_count"]).all()
    ic = rows["index_count"].astype(np.int64).reshape(16, 4)
    assert (ic % 3 == 0).all() and (ic >= 3).all() and (ic[:, 1:] <= ic[:, :-1]).all() and (ic[:, 3] < ic[:, 0]).all()
    assert (rows["base_index"][1:] == np.cumsum(rows["index_count"].astype(np.int64))[:-1]).all()    # consecutive, no overlap
    one_rows, one = synth.lod_groups(meshes, 1, switch_size=())
    assert one_rows["index_count"].tobytes() == meshes["index_count"].tobytes() and (one["first_row"] == np.arange(16)).all()
    with pytest.raises(ValueError):
        synth.lod_groups(meshes, 9)
    # the float64 estimate tracks the twin closely enough to choose thresholds from
    cam = L.camera()
    inst = L.K.cloud(20_000)
    P = L.params(cam)
    est = synth.lod_size_estimate(cam, groups, inst, P["scale"], P["min_distance"])
    exact = L.twin(cam, P, groups, len(rows), inst)["size"].astype(np.float64)
    ok = np.isfinite(exact) & (exact > 0)
    assert ok.sum() > 19_000 and np.max(np.abs(est[ok] / exact[ok] - 1.0)) < 1e-3
