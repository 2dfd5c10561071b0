"""pass::EmitDraws::record_lod / record_batched_lod and MeshPool::add_lods of the C++ mirror (include/voidin.hpp): the host
compiles against the C ABI without a GPU and, with one, writes the lists of a scene from tests/lod_cases.py, which must equal
the ctypes path's and the expected ones byte for byte."""
import os
import subprocess

import numpy as np
import pytest

import lod_cases as L
from conftest import ROOT
from voidin_amd import abi

NAME = "lod_mirror_test"


def build_mirror(directory):
    src = os.path.join(ROOT, "tests", "cpp", NAME + ".cpp")
    exe = os.path.join(directory, NAME)
    lib_dir = os.path.join(ROOT, "voidin_amd", "csrc")
    abi.load()
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), src,
                        "-L", lib_dir, "-lvoidin_hip", f"-Wl,-rpath,{lib_dir}", "-o", exe], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_lod_mirror_compiles_and_links(tmp_path):
    assert os.path.exists(build_mirror(str(tmp_path)))


@pytest.mark.gpu
def test_record_lod_through_the_mirror_equals_the_ctypes_path(ctx, oracle, tmp_path):
    import torch
    n = 50_000
    cam, P, base, meshes, groups, inst = L.scene(oracle, n, 64, 0.2)
    e = L.expect(oracle, cam, P, base, meshes, groups, inst)
    assert 0 < len(e["list"]) < int(e["F"].sum()) < n
    cam1 = np.ascontiguousarray(cam, dtype=abi.CAMERA).reshape(1)
    params = np.zeros(1, abi.LOD_PARAMS)
    params["scale"], params["min_distance"], params["min_size"] = P["scale"], P["min_distance"], P["min_size"]
    src, dst = str(tmp_path / "scene.bin"), str(tmp_path / "result.bin")
    with open(src, "wb") as f:
        f.write(np.array([len(groups), len(meshes), n, 0], np.uint32).tobytes() + cam1.tobytes() + params.tobytes() + groups.tobytes() +
                meshes.tobytes() + inst.tobytes())
    exe = build_mirror(str(tmp_path))
    r = subprocess.run(["timeout", "300", exe, src, dst], capture_output=True, text=True, timeout=400)
    assert r.returncode == 0 and "lod mirror ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    blob = open(dst, "rb").read()
    # the ctypes path
    d_g, d_m, d_i = ctx.upload(groups), ctx.upload(meshes), ctx.upload(inst)
    d_out, d_cmds, d_ids = ctx.empty(n * 20), ctx.empty(len(meshes) * 20), ctx.empty(n * 4)
    d_cnt = torch.zeros(4, dtype=torch.int32, device=ctx.torch_device)
    ctx.cull_compact_lod_dev(cam, params, d_g, len(groups), d_m, len(meshes), d_i, n, d_out, d_cnt[0:1])
    ctx.cull_batch_lod_dev(cam, params, d_g, len(groups), d_m, len(meshes), d_i, n, d_cmds, d_ids, d_cnt[1:2])
    torch.cuda.synchronize()
    k, kb = (int(x) for x in d_cnt.cpu().numpy()[:2])
    ctypes_blob = (np.array([k, kb], np.uint32).tobytes() + d_out.cpu().numpy()[: 20 * k].tobytes() +
                   d_cmds.cpu().numpy()[: 20 * len(meshes)].tobytes() + d_ids.cpu().numpy()[: 4 * kb].tobytes())
    assert blob == ctypes_blob
    assert blob == np.array([len(e["list"]), len(e["ids"])], np.uint32).tobytes() + e["list"].tobytes() + e["cmds"].tobytes() + e["ids"].tobytes()
