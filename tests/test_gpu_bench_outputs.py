"""bench.py on the GPU without --full, and --dump-outputs: a plain run prints the headline keys only; the list it dumps is the
list of its last timed step - the list --full checks against the oracle and hashes - and the same from run to run."""
import os
import zlib

import numpy as np
import pytest

from test_gpu_bench_ranks import _bench

pytestmark = pytest.mark.gpu


def test_plain_run_and_dumped_outputs(tmp_path):
    common = ["--instances", "300001", "--steps", "2", "--warmup", "1"]     # three steps: the last reads the first buffer, the one --full checks
    full = _bench(*common, "--full", "--no-extra", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "full"))
    plain = _bench(*common, "--dump-outputs", str(tmp_path / "plain"))
    for k in ("metric", "unit", "higher_is_better", "dtype"):
        assert plain[k] == full[k], k
    assert plain["value"] > 0 and plain["ms_per_step"] > 0
    assert plain["steps"] == 2 and plain["warmup"] == 1
    assert "roofline" in full and not {"roofline", "cpu_baseline", "extra", "scaling_ceiling"} & set(plain)
    assert full["config"]["verified_bit_exact_vs_oracle"] is True
    files = sorted(os.listdir(tmp_path / "full"))
    assert files == ["draw_count.npy", "draw_rows.npy", "draws.npy"] == sorted(os.listdir(tmp_path / "plain"))
    for f in files:
        assert open(tmp_path / "full" / f, "rb").read() == open(tmp_path / "plain" / f, "rb").read(), f
    count = int(np.load(tmp_path / "full" / "draw_count.npy")[0])
    draws = np.load(tmp_path / "full" / "draws.npy")
    assert 0 < count < 300001 and draws.shape == (count, 5)          # the whole list: count < DUMP_ROWS
    assert zlib.crc32(draws.astype(np.int64).astype(np.uint32).tobytes()) == full["config"]["draw_list_crc32"]
