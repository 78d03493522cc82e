"""Host side of the optimiser selection (sgd / momentum / adam / adamw, per-tensor clipping): the cyclical momentum of
the reference's utils.py:139-204 at hand-computed points, the selection of net.py:1224-1255, the trainer's argument
validation (before anything touches a device), the command-line flags and the refusals of the two C entries, which
return before any launch."""
import ctypes as C

import pytest

from src.training_schedules import LONG_SCHEDULE, SCHEDULES, cyclic_momentum, momentum_value


# ------------------------------------------------------------------------------------------------ cyclic_momentum
@pytest.mark.parametrize("step,kwargs,want", [
    (0, {}, 0.95),                               # the cycle starts at the maximum
    (50, {}, 0.90),
    (100, {}, 0.85),                             # the minimum where the rate peaks
    (150, {}, 0.90),
    (200, {}, 0.95),
    (300, {"mode": "triangular2"}, 0.90),        # second cycle: half the amplitude
    (250, {"one_cycle": True}, 0.95),            # the annealing phase holds the maximum
    (100, {"mode": "exponential"}, 0.95 - 0.1 * 0.99994 ** 100),
])
def test_cyclic_momentum_at_hand_computed_points(step, kwargs, want):
    got = cyclic_momentum(step, 0.85, 0.95, 100, **kwargs)
    assert abs(got - want) <= 1e-12, (got, want)


def test_cyclic_momentum_one_cycle_ignores_the_decays():
    # neither the halving nor gamma applies under one_cycle (utils.py:194-197)
    for mode in ("triangular", "triangular2", "exponential"):
        assert abs(cyclic_momentum(100, 0.85, 0.95, 100, mode=mode, one_cycle=True) - 0.85) <= 1e-12


def test_cyclic_momentum_refuses_an_unknown_mode():
    with pytest.raises(ValueError):
        cyclic_momentum(0, 0.85, 0.95, 100, mode="sawtooth")


# ------------------------------------------------------------------------------------------------ selection
def test_fixed_momentum_wins_over_cyclical():
    for name in ("clr", "one_cycle", "long_schedule"):
        assert momentum_value(SCHEDULES[name], 77, {"clr_stepsize": 100}, momentum=0.5) == 0.5


def test_cyclical_momentum_follows_the_policy():
    p = {"clr_stepsize": 100}
    assert abs(momentum_value(SCHEDULES["clr"], 100, p) - 0.85) <= 1e-12
    assert abs(momentum_value(SCHEDULES["clr"], 250, p) - 0.90) <= 1e-12          # clr: a second triangle
    assert abs(momentum_value(SCHEDULES["one_cycle"], 250, p) - 0.95) <= 1e-12    # one_cycle: held at the maximum
    assert abs(momentum_value(SCHEDULES["one_cycle"], 50, p, None, 0.8, 0.9) - 0.85) <= 1e-12
    # LR range test: one decreasing half cycle over the iterations of the test
    rt = SCHEDULES["lr_range_test"]
    assert abs(momentum_value(rt, 0, p) - 0.95) <= 1e-12
    assert abs(momentum_value(rt, rt["max_iters"] / 2, p) - 0.90) <= 1e-12
    assert abs(momentum_value(rt, rt["max_iters"], p) - 0.85) <= 1e-12


def test_cyclical_momentum_on_a_piecewise_schedule_raises():
    with pytest.raises(ValueError, match="--momentum"):
        momentum_value(LONG_SCHEDULE, 0)


# ------------------------------------------------------------------------------------------------ constructor
def _trainer(**kw):
    from src.trainer import FlowNetSTrainer
    return FlowNetSTrainer(None, 1, 128, 128, **kw)


def test_trainer_refuses_bad_optimizer_arguments_before_touching_the_gpu(monkeypatch):
    from src import trainer

    def no_engine(*a, **k):
        raise AssertionError("the engine must not be built before the arguments are validated")
    monkeypatch.setattr(trainer, "Engine", no_engine)
    with pytest.raises(ValueError, match="optimizer"):
        _trainer(optimizer="lion")
    with pytest.raises(ValueError, match="weight_decay"):
        _trainer(optimizer="adamw", weight_decay=-1e-4)
    for bad in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError, match="momentum"):
            _trainer(optimizer="momentum", momentum=bad)
    with pytest.raises(ValueError, match="--momentum"):        # cyclical momentum on the (default) piecewise schedule
        _trainer(optimizer="momentum")
    with pytest.raises(ValueError, match="clip_grad_norm"):
        _trainer(clip_grad_norm=float("nan"))


def test_valid_optimizer_arguments_reach_the_engine(monkeypatch):
    """clip_grad_norm <= 0 means disabled and is no error; what follows the validation is the engine."""
    from src import trainer

    class Reached(Exception):
        pass

    def engine(*a, **k):
        raise Reached()
    monkeypatch.setattr(trainer, "Engine", engine)
    for kw in (dict(), dict(clip_grad_norm=0), dict(clip_grad_norm=-1.0), dict(optimizer="sgd", clip_grad_norm=2.0),
               dict(optimizer="momentum", momentum=0.9, weight_decay=1e-3), dict(optimizer="adamw"),
               dict(optimizer="momentum", schedule=SCHEDULES["one_cycle"]), dict(optimizer="ADAM")):
        with pytest.raises(Reached):
            _trainer(**kw)


# ------------------------------------------------------------------------------------------------ command lines
NEW_DEFAULTS = dict(optimizer=None, momentum=None, min_momentum=0.85, max_momentum=0.95, weight_decay=None,
                    clip_grad_norm=-1.0)


def test_image_pair_cli_accepts_the_optimizer_flags():
    from src.flownet_s import train as cli
    ap = cli.build_parser()
    f = ap.parse_args(["--list", "x", "--out", "y"])
    for k, v in NEW_DEFAULTS.items():
        assert getattr(f, k) == v, k
    assert (f.training_schedule, f.steps, f.batch, f.dtype, f.clr_stepsize) == ("long_schedule", 1000, 8, "f16x2", None)
    assert cli.optimizer_kwargs(f)["optimizer"] == "adam"
    f = ap.parse_args(["--list", "x", "--out", "y", "--optimizer", "momentum", "--momentum", "0.9", "--min_momentum", "0.8",
                       "--max_momentum", "0.9", "--weight_decay", "1e-3", "--clip_grad_norm", "5"])
    assert cli.optimizer_kwargs(f) == dict(optimizer="momentum", momentum=0.9, min_momentum=0.8, max_momentum=0.9,
                                           weight_decay=1e-3, clip_grad_norm=5.0)
    with pytest.raises(SystemExit):
        ap.parse_args(["--list", "x", "--out", "y", "--optimizer", "lion"])


def test_interp_cli_accepts_the_optimizer_and_schedule_flags():
    from src.flownet_s.train import optimizer_kwargs, schedule_of
    from src.flownet_s_interp import train as cli
    ap = cli.build_parser()
    f = ap.parse_args(["--records", "x", "--out", "y"])
    for k, v in NEW_DEFAULTS.items():
        assert getattr(f, k) == v, k
    assert (f.training_schedule, f.steps, f.batch, f.dtype, f.add_hard_flow_mining) == ("long_schedule", 1000, 8, "f16x2", "")
    assert schedule_of(f) == (LONG_SCHEDULE, {}) and optimizer_kwargs(f)["optimizer"] == "adam"
    f = ap.parse_args(["--records", "x", "--out", "y", "--optimizer", "adamw", "--training_schedule", "one_cycle",
                       "--clr_min_lr", "1e-6", "--clr_max_lr", "1e-3", "--clr_stepsize", "500", "--clr_gamma", "0.9",
                       "--clr_mode", "triangular", "--one_cycle_annealing_factor", "0.01", "--start_lr", "1e-8",
                       "--end_lr", "0.5", "--clip_grad_norm", "1.0"])
    sched, params = schedule_of(f)
    assert sched is SCHEDULES["one_cycle"] and params["clr_stepsize"] == 500 and len(params) == 8
    assert optimizer_kwargs(f)["clip_grad_norm"] == 1.0 and f.optimizer == "adamw"


def test_a_namespace_without_the_new_flags_means_adam():
    import types
    from src.flownet_s.train import optimizer_kwargs, schedule_of
    old = types.SimpleNamespace(batch=2)
    assert optimizer_kwargs(old) == dict(optimizer="adam", momentum=None, min_momentum=0.85, max_momentum=0.95,
                                         weight_decay=None, clip_grad_norm=-1.0)
    assert schedule_of(old) == (LONG_SCHEDULE, {})


# ------------------------------------------------------------------------------------------------ C ABI refusals
def test_optimizer_entries_refuse_bad_arguments_without_a_launch():
    """Null table, n_tensors outside 1..65535 and an unknown kind: FN2_ERR_INVALID_ARGUMENT, returned before any launch
    (so this runs without a device; the pointers are never dereferenced on the host)."""
    from src import _hip
    lib = _hip.lib()
    buf = (C.c_float * 256)()
    p = C.cast(buf, C.c_void_p)
    bad = _hip.ERR_INVALID_ARGUMENT
    assert lib.fn2_optim_grad_sumsq_multi(None, p, p, 1, p, p, None) == bad
    assert lib.fn2_optim_grad_sumsq_multi(p, p, p, 0, p, p, None) == bad
    assert lib.fn2_optim_grad_sumsq_multi(p, p, p, 65536, p, p, None) == bad
    assert lib.fn2_optim_grad_sumsq_multi(p, p, p, 1, p, None, None) == bad
    for kind in _hip.OPTIM_KINDS.values():
        assert lib.fn2_optim_step_multi_dev(kind, None, p, p, 1, p, None, None) == bad
        assert lib.fn2_optim_step_multi_dev(kind, p, p, p, 0, p, None, None) == bad
        assert lib.fn2_optim_step_multi_dev(kind, p, p, p, 65536, p, None, None) == bad
        assert lib.fn2_optim_step_multi_dev(kind, p, p, p, 1, None, None, None) == bad
    for kind in (-1, 4, 99):
        assert lib.fn2_optim_step_multi_dev(kind, p, p, p, 1, p, None, None) == bad
    assert b"kind" in lib.fn2_last_error()
    assert sorted(_hip.OPTIM_KINDS.items(), key=lambda kv: kv[1]) == [("sgd", 0), ("momentum", 1), ("adam", 2), ("adamw", 3)]
