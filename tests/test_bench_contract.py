"""bench.py's command line and leg table, checked without a GPU: the driver runs `python bench.py --gpus N --steps K --warmup W` and the
line's legs are spelled as argument overrides -- a typo in one would only show on the GPU box."""
import copy
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_defaults_and_legs_are_well_formed():
    import bench
    a = bench.parse_defaults()
    assert a.gpus == 1 and a.steps >= 10 and a.warmup >= 1 and a.ndim == 100 and a.ntemps == 64 and a.nwalkers == 4096
    assert a.mix == "scam" and a.logl == "iso" and a.cov_mode == "pooled" and not a.callback
    names = [n for n, _, _, _ in bench.ALSO]
    assert len(names) == len(set(names)) and "config2_batched_callback" in names and "config4_share_1000d_64x512" in names
    parser = bench.make_parser()
    choices = {act.dest: act.choices for act in parser._actions if act.choices}
    for name, over, steps, warmup in bench.ALSO:
        b = copy.copy(a)
        for k, v in over.items():
            assert hasattr(b, k), (name, k)                              # every override is an argument of the parser
            if k in choices:
                assert v in choices[k], (name, k, v)
            setattr(b, k, v)
        assert steps >= 1 and warmup >= 1
        w = bench.cycle_weights(b)
        assert len(w) == 3 and sum(w) > 0
        if b.mix == "default" and not b.callback:
            assert warmup > 100                                          # DE joins the cycle after burn = 10000 iterations = 100 steps


def test_the_drivers_command_line_parses():
    import bench
    a = bench.make_parser().parse_args(["--gpus", "8", "--steps", "20", "--warmup", "5"])
    assert (a.gpus, a.steps, a.warmup) == (8, 20, 5) and a.partition == "temps"
    assert bench.TSKIP == 100 and bench.HBM_PEAK_GBS == 8000.0


def test_plain_run_and_full_options():
    import bench
    a = bench.parse_defaults()
    assert a.full is False and a.dump_outputs is None
    a = bench.make_parser().parse_args(["--steps", "3", "--warmup", "0", "--full", "--dump-outputs", "out"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (3, 0, True, "out")


class _HostEngine(object):
    """The attributes of PTEngine that bench.dump_outputs reads, on CPU tensors."""

    def __init__(self, W, nt, d, per_walker, seed=0):
        import numpy as np
        import torch
        rng = np.random.default_rng(seed)
        self.W, self.nt, self.d, self.ntg, self.Wc = W, nt, d, nt, W if per_walker else 1
        self.device = torch.device("cpu")
        slot = np.stack([rng.permutation(nt) for _ in range(W)]).astype(np.int32)
        temp = np.argsort(slot, axis=1).astype(np.int32)
        self.t = dict(X=torch.from_numpy(rng.standard_normal((W, nt, d))), lnL=torch.from_numpy(rng.standard_normal((W, nt))),
                      lp=torch.from_numpy(rng.standard_normal((W, nt))), slot_of=torch.from_numpy(slot), temp_of=torch.from_numpy(temp),
                      nacc=torch.from_numpy(rng.integers(0, 1000, (W, nt))), nswap=torch.from_numpy(rng.integers(0, 1000, (W, nt))),
                      cov=torch.from_numpy(rng.standard_normal((self.Wc, d, d))))

    def get(self, name):
        return self.t[name].numpy()

    def by_temp(self, name):
        import numpy as np
        a, so = self.get(name), self.get("slot_of").astype(np.int64)
        return np.take_along_axis(a, so.reshape(so.shape + (1,) * (a.ndim - 2)), 1)


def test_dump_outputs_writes_the_state_in_temperature_order(tmp_path):
    import numpy as np
    import bench
    eng = _HostEngine(W=6, nt=5, d=3, per_walker=False)
    assert bench.dump_outputs(eng, str(tmp_path)) == 6                  # small enough: every walker
    got = {n: np.load(str(tmp_path / (n + ".npy"))) for n in ("walkers", "X", "lnL", "lp", "nacc", "nswap", "cov")}
    assert all(v.dtype == np.float64 for v in got.values())
    assert np.array_equal(got["walkers"], np.arange(6))
    for name in ("X", "lnL", "lp"):
        assert np.array_equal(got[name], eng.by_temp(name))
    for name in ("nacc", "nswap", "cov"):
        assert np.array_equal(got[name], eng.get(name).astype(np.float64))


def test_dump_outputs_samples_a_fixed_set_of_walkers_within_the_budget(tmp_path, monkeypatch):
    import numpy as np
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", 40000)
    eng = _HostEngine(W=200, nt=4, d=8, per_walker=True)
    nw = bench.dump_outputs(eng, str(tmp_path / "a"))
    assert 1 <= nw < 200
    assert sum(f.stat().st_size - 128 for f in (tmp_path / "a").iterdir()) <= 40000     # (128: the header of a .npy file)
    ws = np.load(str(tmp_path / "a" / "walkers.npy")).astype(np.int64)
    assert len(ws) == nw and np.all(np.diff(ws) > 0)
    X, cov = np.load(str(tmp_path / "a" / "X.npy")), np.load(str(tmp_path / "a" / "cov.npy"))
    assert np.array_equal(X, eng.by_temp("X")[ws]) and np.array_equal(cov, eng.get("cov")[ws])
    # the same walkers for another state of the same shape: two builds are compared row for row
    assert bench.dump_outputs(_HostEngine(W=200, nt=4, d=8, per_walker=True, seed=1), str(tmp_path / "b")) == nw
    assert np.array_equal(np.load(str(tmp_path / "b" / "walkers.npy")), ws)
