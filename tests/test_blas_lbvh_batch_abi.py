"""The batched LBVH bottom level without a device: the item record against the header, and every call that must fail before it
touches a device.  vd_bvh_lbvh_plan_dev judges its items BEFORE it looks at the context, so every refusal that names an item can
be seen here with a null context and pointers that are never followed; the same cases with a live context (which then returns
no plan), and n_items == 0 == VD_OK, are in tests/test_gpu_blas_lbvh_batch.py."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT
from voidin_amd import abi

FAKE = 1 << 20          # 16-byte aligned, never followed


def _items(caps, **bad):
    """Valid items of the given capacities; bad: field -> (item, value)."""
    items = (abi.BvhLbvhBatchItem * len(caps))()
    for m, cap in enumerate(caps):
        items[m].verts_xyz, items[m].indices_inout, items[m].nodes, items[m].mesh_info = FAKE, FAKE, FAKE, None
        items[m].n_vert, items[m].tri_cap, items[m].node_cap, items[m].status = 3, cap, max(2, 2 * cap), 77
    for field, (m, value) in bad.items():
        setattr(items[m], field, value)
    return items


def test_item_layout_is_the_headers():
    """Size and offsets from a C11 compile of the header itself."""
    import subprocess
    import tempfile
    assert C.sizeof(abi.BvhLbvhBatchItem) == 48 == abi.BVH_LBVH_BATCH_ITEM.itemsize
    fields = [name for name, _ in abi.BvhLbvhBatchItem._fields_]
    assert fields == list(abi.BVH_LBVH_BATCH_ITEM.names)
    checks = " && ".join(f"offsetof(VdBvhLbvhBatchItem, {f}) == {getattr(abi.BvhLbvhBatchItem, f).offset}" for f in fields)
    for f in fields:
        assert getattr(abi.BvhLbvhBatchItem, f).offset == abi.BVH_LBVH_BATCH_ITEM.fields[f][1]
    src = ('#include <stddef.h>\n#include "voidin_abi.h"\n'
           f'_Static_assert(sizeof(VdBvhLbvhBatchItem) == 48 && {checks}, "item layout");\n'
           f'_Static_assert(VD_BVH_LBVH_BATCH_MAX_ITEMS == {abi.BVH_LBVH_BATCH_MAX_ITEMS}u, "constant");\n'
           "int main(void) { return 0; }\n")
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "item.c")
        open(p, "w").write(src)
        r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), p], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]


def test_null_ctx_is_an_error_not_a_crash():
    lib = abi.load()
    items = _items([4, 5])
    out = C.c_void_p(0x1234)
    assert lib.vd_bvh_lbvh_plan_dev(None, C.addressof(items), 2, C.byref(out)) == abi.VD_ERR_INVALID_ARG
    assert out.value is None and [it.status for it in items] == [0, 0]          # good items, no context: no plan
    assert lib.vd_bvh_lbvh_plan_dev(None, None, 0, C.byref(out)) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_bvh_lbvh_plan_dev(None, C.addressof(items), 2, None) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_bvh_build_lbvh_planned_dev(None, None, None, None) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_bvh_build_lbvh_planned_dev(None, FAKE, FAKE, FAKE) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_bvh_lbvh_plan_release(None, None) == abi.VD_ERR_INVALID_ARG
    assert lib.vd_bvh_build_lbvh_batch(None, C.addressof(items), 2, None, FAKE) == abi.VD_ERR_INVALID_ARG


BAD_ITEMS = {
    "null verts": dict(verts_xyz=(1, None)),
    "null indices": dict(indices_inout=(2, None)),
    "null nodes": dict(nodes=(0, None)),
    "tri_cap 0": dict(tri_cap=(1, 0)),
    "node_cap below 2 tri_cap": dict(node_cap=(2, 2 * 700 - 1)),
    "node_cap below 2": dict(tri_cap=(0, 1), node_cap=(0, 1)),
    "nodes not 16-byte aligned": dict(nodes=(1, FAKE + 8)),
}


@pytest.mark.parametrize("case", sorted(BAD_ITEMS))
def test_plan_refuses_a_bad_item_and_names_it(case):
    lib = abi.load()
    bad = BAD_ITEMS[case]
    items = _items([300, 5, 700], **bad)
    culprit = {m for m, _ in bad.values()}
    assert len(culprit) == 1
    m = culprit.pop()
    out = C.c_void_p(0x1234)
    assert lib.vd_bvh_lbvh_plan_dev(None, C.addressof(items), 3, C.byref(out)) == abi.VD_ERR_INVALID_ARG
    assert out.value is None
    assert items[m].status == abi.VD_ERR_INVALID_ARG
    assert all(items[k].status == 0 for k in range(3) if k != m)


def test_plan_refuses_too_many_items_and_too_many_slots():
    lib = abi.load()
    out = C.c_void_p(0x1234)
    n = abi.BVH_LBVH_BATCH_MAX_ITEMS + 1
    items = _items([1] * n)
    assert lib.vd_bvh_lbvh_plan_dev(None, C.addressof(items), n, C.byref(out)) == abi.VD_ERR_INVALID_ARG
    assert out.value is None and items[0].status == 77 and items[n - 1].status == 77       # refused as a whole: no item was judged
    # the capacities add up past VD_BVH_LBVH_MAX_TRIANGLES: the item that crosses it is named
    half = abi.BVH_LBVH_MAX_TRIANGLES // 2
    items = _items([half, half, 1])
    assert lib.vd_bvh_lbvh_plan_dev(None, C.addressof(items), 3, C.byref(out)) == abi.VD_ERR_INVALID_ARG
    assert [it.status for it in items] == [0, 0, abi.VD_ERR_INVALID_ARG]
    items = _items([abi.BVH_LBVH_MAX_TRIANGLES + 1])
    assert lib.vd_bvh_lbvh_plan_dev(None, C.addressof(items), 1, C.byref(out)) == abi.VD_ERR_INVALID_ARG
    assert items[0].status == abi.VD_ERR_INVALID_ARG


def test_header_states_the_clamp_and_the_empty_mesh():
    text = open(os.path.join(ROOT, "include", "voidin_abi.h")).read()
    flat = re.sub(r"\s*\n \*\s*", " ", text)
    assert "ABOVE THE CAPACITY IS READ AS THE CAPACITY" in flat and "T_m == 0" in flat
