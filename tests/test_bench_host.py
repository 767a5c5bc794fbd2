"""CPU: host logic of bench.py -- the N>1 self-launch (a CHILD torchrun, never exec), the --gpus /
WORLD_SIZE check, the host-core count."""
import os
import subprocess
import sys
import types

import pytest

from conftest import ROOT


def _bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench


def test_self_launch_starts_child_torchrun_and_relays_its_code(monkeypatch):
    bench = _bench()
    seen = {}

    def fake_run(cmd, env=None, **kw):
        seen["cmd"], seen["env"] = cmd, env
        return types.SimpleNamespace(returncode=7)
    monkeypatch.setattr(subprocess, "run", fake_run)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3", "--warmup", "1"])
    with pytest.raises(SystemExit) as e:
        bench.self_launch(types.SimpleNamespace(gpus=4))
    assert e.value.code == 7                                       # non-zero child -> non-zero parent
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in cmd and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-6:] == ["--gpus", "4", "--steps", "3", "--warmup", "1"]
    assert os.path.basename(cmd[-7]) == "bench.py"
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_gpus_must_match_world_size(monkeypatch):
    bench = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert "does not match WORLD_SIZE" in str(e.value)


def test_host_cores_is_positive_and_uncapped():
    bench = _bench()
    n = bench.host_cores()
    assert 1 <= n <= (os.cpu_count() or 1)


def test_plain_run_is_headline_only_by_default(monkeypatch):
    bench = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse_args()
    assert a.steps == 3 and a.warmup == 1 and a.full is False and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse_args()
    assert a.full is True and a.dump_outputs == "d"


@pytest.mark.parametrize("B", [2, 32])
def test_dump_outputs_float_arrays_within_budget(B, tmp_path):
    """--dump-outputs on host tensors shaped like a search result: records decoded, every file float32 / float64,
    the Grad-CAM maps whole when they fit and a fixed seeded sample when they do not."""
    import numpy as np
    import torch
    import ivf_search
    bench = _bench()
    T = 16
    g = torch.Generator().manual_seed(1)
    res = {k: torch.rand(B, generator=g) for k in ivf_search.RECORD_FLOAT_FIELDS}
    res.update(pred_class=torch.randint(0, 174, (B,), generator=g), target=torch.randint(0, 174, (B,), generator=g),
               time_mask=torch.rand(B, T, generator=g), init_mask=torch.rand(B, T, generator=g) * 10 - 5,
               ranking=torch.argsort(torch.rand(B, T, generator=g), dim=1),
               gradcam=torch.rand(B, T, 224, 224, generator=g))
    res["snapped"] = res["time_mask"] > 0.5
    rec = ivf_search.pack_records(list(range(10, 10 + B)), res, T)
    bench.dump_outputs(torch, str(tmp_path), res, rec, T)
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert sum((tmp_path / f).stat().st_size for f in os.listdir(tmp_path)) <= bench.DUMP_BYTES
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert got["clip_id"].tolist() == list(range(10, 10 + B))
    for k in ("pred_class", "target", "ranking", "time_mask", "init_mask", "snapped") + ivf_search.RECORD_FLOAT_FIELDS:
        assert np.array_equal(got[k], res[k].numpy().astype(got[k].dtype)), k
    if B == 2:
        assert np.array_equal(got["gradcam"], res["gradcam"].numpy()) and "gradcam_sample" not in got
    else:
        s = got["gradcam_sample"]
        assert "gradcam" not in got and s.shape == (bench.DUMP_CAM_ELEMS,)
        assert np.all(np.isin(s[:1000], res["gradcam"].numpy()))


def test_headline_kernel_choice_record_fits_only_its_plan(tmp_path, monkeypatch):
    """The committed headline choice loads for the default plan of the built library's variant table and for nothing
    else (other plans run the built-in choice); a missing or malformed file is no choice."""
    import json
    import ivf_lib
    bench = _bench()
    doc = json.load(open(bench.TUNING_FILE))
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    a = bench.parse_args()
    assert (doc["batch"], doc["frames"], doc["math"]) == (a.batch, a.frames, a.math)
    v = ivf_lib.lib().ivf_version()
    assert doc["lib_version"] == v
    assert bench.read_tuning(bench.TUNING_FILE, 32, "bf16x6", 16, v) == doc["variants"]
    for B, m, T, ver in ((2, "bf16x6", 16, v), (32, "bf16x3", 16, v), (32, "bf16x6", 32, v), (32, "bf16x6", 16, v + 1)):
        assert bench.read_tuning(bench.TUNING_FILE, B, m, T, ver) is None
    assert bench.read_tuning(str(tmp_path / "missing.json"), 32, "bf16x6", 16, v) is None
    (tmp_path / "bad.json").write_text("{")
    assert bench.read_tuning(str(tmp_path / "bad.json"), 32, "bf16x6", 16, v) is None
