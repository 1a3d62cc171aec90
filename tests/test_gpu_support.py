"""CPU: tests/gpu_support.py, the helper the GPU tests, the rank workers and the timing tools share -- the scene model, the
exporter's base arguments, the 1-rank patch, the launcher's environment, and a launch of two CPU ranks whose failure must
surface the worker's own traceback."""
import os

import numpy as np
import pytest
import torch

from nerfmeshes_amd import dist as nd, synthetic as S
from tests import gpu_support as gs


def test_scene_model_holds_the_scene_weights_in_both_networks():
    model = gs.scene_model("cpu", chunksize=3000, train_perturb=True)
    sd = model.state_dict()
    for prefix in ("model_coarse.", "model_fine."):
        for k, v in S.make_scene_weights().items():
            got = sd[prefix + k].numpy()
            assert got.dtype == v.dtype and got.shape == v.shape and got.tobytes() == v.tobytes(), prefix + k
    assert not model.training and not model.model_coarse.training and not model.model_fine.training
    assert model.cfg.nerf.validation.chunksize == 3000 and model.cfg.nerf.train.chunksize == 3000
    assert model.cfg.nerf.train.perturb is True and model.cfg.nerf.validation.perturb is False
    assert next(model.parameters()).device.type == "cpu"


def test_export_args_base_and_overrides(tmp_path):
    args = gs.export_args(tmp_path, "--res", "24", "--iso-level", "16")
    assert args.save_dir == str(tmp_path) and args.view_disparity_max_bound == 1.0 and args.batch_size == 4096
    assert args.iso_level == 16 and args.res == 24, "what the caller passes comes last and wins"
    assert gs.export_args(tmp_path).iso_level == 32


def test_single_rank_patches_and_restores():
    real = nd.world, nd.all_gather_rows, nd.all_gather_ragged
    x, counts = torch.arange(6.0).reshape(2, 3), [2]

    def inside():
        assert nd.world() == (0, 1) and nd.all_gather_rows(x, counts) is x
        assert nd.all_gather_ragged is real[2], "only the named collective is replaced"
        return "done"

    assert gs.single_rank(inside) == "done"
    assert (nd.world, nd.all_gather_rows, nd.all_gather_ragged) == real

    def raising():
        assert nd.world() == (0, 1) and nd.all_gather_ragged(x) is x and nd.all_gather_rows is real[1]
        raise KeyError("inside")

    with pytest.raises(KeyError, match="inside"):
        gs.single_rank(raising, gather="all_gather_ragged")
    assert (nd.world, nd.all_gather_rows, nd.all_gather_ragged) == real


def test_clean_env_drops_the_rendezvous(monkeypatch):
    for k in gs.RENDEZVOUS:
        monkeypatch.setenv(k, "7")
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", "1")
    before = dict(os.environ)
    env = gs.clean_env(FOO="1")
    assert set(gs.RENDEZVOUS) == {"RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"}
    assert not set(gs.RENDEZVOUS) & set(env)
    assert env["HSA_ENABLE_IPC_MODE_LEGACY"] == "0" and env["FOO"] == "1"
    assert dict(os.environ) == before and "FOO" not in os.environ
    assert {k: v for k, v in env.items() if k not in ("FOO", "HSA_ENABLE_IPC_MODE_LEGACY")} == \
        {k: v for k, v in before.items() if k not in gs.RENDEZVOUS + ("HSA_ENABLE_IPC_MODE_LEGACY",)}


def test_to_numpy_and_quiet(capsys):
    assert gs.to_numpy(None) is None and np.array_equal(gs.to_numpy(torch.arange(3)), [0, 1, 2])
    with gs.quiet():
        print("not shown")
    assert capsys.readouterr().out == ""


GOOD = """import os
if os.environ["RANK"] == "0":
    print("CPU_RANKS_OK world=" + os.environ["WORLD_SIZE"], flush=True)
"""
BAD = """import os
if os.environ["RANK"] == "1":
    raise RuntimeError("rank one says no")
"""


def test_launch_ranks_on_two_cpu_ranks(tmp_path):
    script = tmp_path / "good.py"
    script.write_text(GOOD)
    r = gs.launch_ranks(str(script), 2, ranks_per_gpu=False, timeout=120)
    gs.assert_ranks_ok(r, "CPU_RANKS_OK world=2")


def test_launch_ranks_puts_the_workers_traceback_in_front(tmp_path):
    script = tmp_path / "bad.py"
    script.write_text(BAD)
    r = gs.launch_ranks(str(script), 2, ranks_per_gpu=False, timeout=120)
    assert r.returncode != 0
    head = r.stderr.splitlines()[:40]
    assert head[0].startswith("Traceback") and any("rank one says no" in line for line in head), r.stderr[:3000]
    with pytest.raises(AssertionError, match="rank one says no"):
        gs.assert_ranks_ok(r, "CPU_RANKS_OK")
