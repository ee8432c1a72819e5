"""bench.py's command line without a GPU: what a plain run leaves to --full, the options that need --full, and the 64 MB cap of
--dump-outputs (a fixed, seeded sample of the crops when the outputs are larger)."""
import importlib

import numpy as np
import pytest
import torch


@pytest.mark.parametrize("argv", [["--layers", "layers.csv"], ["--extra", "batch_sweep_hrnet_w32_f32"], ["--steps", "0"],
                                  ["--dump-outputs", "out", "--workload", "hrnet_w32_train"],
                                  ["--dump-outputs", "out", "--sweep", "1,32"]])
def test_options_rejected_before_any_gpu_work(argv):
    bench = importlib.import_module("bench")
    with pytest.raises(SystemExit) as exc:
        bench.parse_args(argv)
    assert exc.value.code == 2  # argparse error: nothing was built or timed


def test_plain_run_leaves_the_extra_measurements_to_full():
    bench = importlib.import_module("bench")
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2", "--dump-outputs", "out"])
    assert (a.steps, a.warmup, a.dump_outputs) == (7, 2, "out")
    assert not a.full and a.no_roofline and a.no_cpu_baseline and a.no_extra
    a = bench.parse_args(["--full", "--no-cpu-baseline", "--layers", "layers.csv"])
    assert a.full and not a.no_roofline and a.no_cpu_baseline and not a.no_extra and a.layers == "layers.csv"


def test_dump_outputs_writes_float32_within_64_mb(tmp_path):
    bench = importlib.import_module("bench")
    g = torch.Generator().manual_seed(0)
    small = {"preds": torch.randn(4, 17, 3, generator=g), "boxes": torch.randn(4, 6, generator=g),
             "heatmap": torch.randn(4, 17, 64, 48, generator=g).half()}
    bench.dump_outputs(str(tmp_path / "small"), small)
    for k, v in small.items():
        a = np.load(tmp_path / "small" / f"{k}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, v.float().numpy())
    assert not list((tmp_path / "small").glob("*_rows.npy"))

    big = {"preds": torch.zeros(512, 17, 3), "boxes": torch.zeros(512, 6),
           "heatmap": torch.arange(512, dtype=torch.float32)[:, None, None, None].expand(512, 17, 64, 48)}
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), big)
    total = sum(np.load(p).nbytes for p in (tmp_path / "a").glob("*.npy"))
    assert total <= 64 << 20
    rows = np.load(tmp_path / "a" / "heatmap_rows.npy")
    hm = np.load(tmp_path / "a" / "heatmap.npy")
    assert rows.dtype == np.float64 and hm.shape[0] == len(rows) < 512 and np.all(np.diff(rows) > 0)
    assert np.array_equal(hm[:, 0, 0, 0], rows.astype(np.float32))  # each kept crop is the crop its row names
    assert np.array_equal(rows, np.load(tmp_path / "b" / "heatmap_rows.npy"))  # the same sample in every run
    assert np.load(tmp_path / "a" / "preds.npy").shape == (512, 17, 3)
