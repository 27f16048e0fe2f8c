"""bench.py command line (CPU): the plain run is the lean default, the extra
legs sit behind --full, and --dump-outputs writes the step result exactly."""
import importlib.util
import os

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location(
        "bench", os.path.join(REPO, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)  # no GPU touched until main()
    return mod


def test_plain_run_is_lean_by_default(bench):
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert (a.gpus, a.steps, a.warmup) == (1, 7, 3)
    assert a.full is False and a.dump_outputs is None
    assert bench.parse_args(["--full"]).full is True
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


def test_dump_outputs_roundtrip(bench, tmp_path, golden):
    point = bytes.fromhex(golden("msm.json")["seeded_cases"][0]["result"])
    out = tmp_path / "nested" / "dump"
    bench.dump_outputs(str(out), point)
    assert sorted(os.listdir(out)) == ["msm_result.npy"]
    arr = np.load(out / "msm_result.npy")
    assert arr.dtype == np.float32 and arr.shape == (64,)
    assert bytes(arr.astype(np.uint8)) == point
