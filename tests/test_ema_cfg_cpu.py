"""CPU: `custom_hooks` / EMAHook on the host -- optim_cfg.check_custom_hooks (accepted forms, defaults, every rejection by name),
ema_coefficient against the reference's expression (mmdet/models/layers/ema.py:64-65), ema_started at its boundaries, the
per-iteration rule, the new config, and the restatement tests/ema_refs.py itself: its one-rounding multiply-add against exact
rational arithmetic, and torch's CPU `mul_(1 - c).add_(src, alpha=c)` within one ulp of it."""
import math
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import ema_refs as E
from erd_amd import Config
from erd_amd import optim_cfg as OC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_EMA = os.path.join(ROOT, "configs", "gfl_increment", "gfl_r50_fpn_1x_coco_first_40_incre_last_40_cats_ema.py")
CFG_INCRE = os.path.join(ROOT, "configs", "gfl_increment", "gfl_r50_fpn_1x_coco_first_40_incre_last_40_cats.py")


def hook(**kw):
    return [dict(type="EMAHook", **kw)]


def test_absent_or_empty_custom_hooks_mean_no_average():
    assert OC.check_custom_hooks(None) is None
    assert OC.check_custom_hooks([]) is None
    assert Config.fromfile(CFG_INCRE).get("custom_hooks") is None, "no other config of the tree has custom_hooks"


def test_defaults_and_accepted_forms():
    d = OC.check_custom_hooks(hook())
    assert d == dict(ema_type="ExponentialMovingAverage", momentum=0.0002, gamma=2000.0, interval=1, update_buffers=False,
                     strict_load=False, begin_iter=0, begin_epoch=0)
    d = OC.check_custom_hooks(hook(ema_type="ExpMomentumEMA", momentum=0.001, gamma=300, interval=3, update_buffers=True, priority=49,
                                   strict_load=True, begin_epoch=2, device=None))
    assert d == dict(ema_type="ExpMomentumEMA", momentum=0.001, gamma=300.0, interval=3, update_buffers=True, strict_load=True,
                     begin_iter=0, begin_epoch=2)
    assert "priority" not in d                                      # accepted and ignored
    assert OC.check_custom_hooks(hook(begin_iter=7, priority="ABOVE_NORMAL"))["begin_iter"] == 7
    # update_buffers is accepted with either value and changes nothing else
    a, b = OC.check_custom_hooks(hook(update_buffers=True)), OC.check_custom_hooks(hook(update_buffers=False))
    assert {k: v for k, v in a.items() if k != "update_buffers"} == {k: v for k, v in b.items() if k != "update_buffers"}
    # ConfigDict entries (what Config.fromfile hands over) pass like plain dicts
    assert OC.check_custom_hooks(Config(dict(custom_hooks=hook(momentum=0.5))).custom_hooks)["momentum"] == 0.5


@pytest.mark.parametrize("bad, name", [
    (hook(ema_type="StochasticWeightAverage"), "ema_type"),
    (hook(ema_type="MomentumAnnealingEMA"), "ema_type"),
    (hook(momentums=0.1), "momentums"),
    (hook(gamma=100), "gamma"),                                     # ExpMomentumEMA only
    (hook(momentum=0.0), "momentum"),
    (hook(momentum=1.0), "momentum"),
    (hook(momentum=-0.1), "momentum"),
    (hook(ema_type="ExpMomentumEMA", gamma=0), "gamma"),
    (hook(ema_type="ExpMomentumEMA", gamma=-5), "gamma"),
    (hook(interval=0), "interval"),
    (hook(interval=1.5), "interval"),
    (hook(begin_iter=3, begin_epoch=1), "begin_iter and begin_epoch"),
    (hook(begin_iter=-1), "begin_iter"),
    (hook(device="cpu"), "device"),
    ([dict(type="SyncNormHook")], "SyncNormHook"),
    (hook() + [dict(type="NumClassCheckHook")], "NumClassCheckHook"),
    (hook() + hook(), "EMAHook"),
])
def test_every_rejection_names_its_key(bad, name):
    with pytest.raises(ValueError, match=name):
        OC.check_custom_hooks(bad)


@pytest.mark.parametrize("momentum", [0.0002, 0.5])
@pytest.mark.parametrize("steps", [1, 2, 1999, 2000, 10 ** 6])
def test_ema_coefficient_is_the_reference_expression(momentum, steps):
    gamma = 2000
    ref = (1 - momentum) * math.exp(-float(1 + steps) / gamma) + momentum             # ema.py:64-65, written out
    assert OC.ema_coefficient("ExpMomentumEMA", momentum, gamma, steps) == ref == E.coefficient("ExpMomentumEMA", momentum, gamma, steps)
    assert OC.ema_coefficient("ExponentialMovingAverage", momentum, gamma, steps) == momentum
    assert momentum <= ref < 1.0
    with pytest.raises(ValueError, match="ema_type"):
        OC.ema_coefficient("SWA", momentum, gamma, steps)


def test_ema_started_at_the_boundaries():
    by_iter = OC.check_custom_hooks(hook(begin_iter=3))
    assert [OC.ema_started(by_iter, it, 0) for it in range(5)] == [False, False, True, True, True]      # iter + 1 >= 3
    assert OC.ema_started(by_iter, 0, 9) is False                   # the epoch does not count when begin_iter is given
    by_epoch = OC.check_custom_hooks(hook(begin_epoch=2))
    assert [OC.ema_started(by_epoch, 10 ** 6, e) for e in range(3)] == [False, True, True]              # epoch + 1 >= 2
    assert OC.ema_started(OC.check_custom_hooks(hook()), 0, 0) is True
    for cfg in (by_iter, by_epoch):
        for it in range(5):
            for ep in range(3):
                assert OC.ema_started(cfg, it, ep) == E.started(cfg, it, ep)


def test_iteration_rule_copy_average_skip_and_the_count():
    cfg = OC.check_custom_hooks(hook(momentum=0.5, interval=2, begin_iter=3))
    steps, seen = 0, []
    for it in range(8):
        mode, c, steps = OC.ema_action(cfg, steps, OC.ema_started(cfg, it, 0))
        seen.append((mode, steps))
        assert c == (0.5 if mode == "average" else 0.0)
    #             not started (steps stays 0)      first started: copy; then steps 1: skip, 2: average, 3: skip, ...
    assert seen == [("copy", 0), ("copy", 0), ("copy", 1), ("skip", 2), ("average", 3), ("skip", 4), ("average", 5), ("skip", 6)]
    exp = OC.check_custom_hooks(hook(ema_type="ExpMomentumEMA", gamma=3))
    steps = 0
    for it in range(6):
        mode, c, new = OC.ema_action(exp, steps, True)
        rmode, rc, rnew = E.action(exp, steps, True)
        assert (mode, new) == (rmode, rnew) and (c == rc if mode == "average" else rc is None)
        if it:
            assert mode == "average" and c == (1 - 0.0002) * math.exp(-(1 + steps) / 3) + 0.0002
        steps = new
    assert steps == 6


def test_the_ema_config_loads_and_resolves():
    cfg = Config.fromfile(CFG_EMA)
    base = Config.fromfile(CFG_INCRE)
    assert cfg.model.to_dict() == base.model.to_dict() and cfg.optim_wrapper.to_dict() == base.optim_wrapper.to_dict()
    d = OC.check_custom_hooks(cfg.custom_hooks)
    assert d == dict(ema_type="ExpMomentumEMA", momentum=0.0002, gamma=2000.0, interval=1, update_buffers=True, strict_load=False,
                     begin_iter=0, begin_epoch=0)


# ---- the restatement itself ---------------------------------------------------------------------------------------------------------
def _round_fraction_to_f32(q):
    """the fp32 nearest to the rational q, ties to even, by exact comparison among the neighbours of a first guess"""
    g = np.float32(float(q))
    cand = sorted({float(np.nextafter(g, np.float32(-np.inf))), float(g), float(np.nextafter(g, np.float32(np.inf)))})
    best = min(cand, key=lambda v: (abs(Fraction(v) - q), int(np.float32(v).view(np.uint32)) & 1))
    return np.float32(best)


def test_fma32_rounds_once_also_where_float64_would_round_twice():
    rng = np.random.RandomState(0)
    a = rng.standard_normal(300).astype(np.float32)
    b = rng.standard_normal(300).astype(np.float32)
    c = (rng.standard_normal(300) * 10.0 ** rng.uniform(-20, 3, 300)).astype(np.float32)
    # crafted: the product is exactly the midpoint of two fp32 neighbours and the addend lies far below one float64 step
    a[:4] = np.float32(1 + 2.0 ** -23)
    b[:4] = np.float32(1.5)
    c[:4] = np.array([2.0 ** -80, -2.0 ** -80, 2.0 ** -120, 0.0], dtype=np.float32)
    got = E.fma32(a, b, c)
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    want = np.array([_round_fraction_to_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not np.array_equal(naive[:2].view(np.uint32), want[:2].view(np.uint32)), "the crafted ties do separate one rounding from two"
    if hasattr(math, "fma"):                                        # (Python >= 3.13 has the C library's fma)
        ref = np.array([np.float32(math.fma(float(x), float(y), float(z))) for x, y, z in zip(a[4:], b[4:], c[4:])])
        assert np.array_equal(got[4:].view(np.uint32), ref.view(np.uint32))


def test_update_special_values_follow_ieee():
    c = 0.25
    ema = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, 3e38, 3e38], dtype=np.float32)
    src = np.array([-0.0, -0.0, 1.0, np.inf, 1.0, 1e-45, 3e38, -3e38], dtype=np.float32)
    out = E.update(ema, src, c)
    assert out[0] == 0.0 and not np.signbit(out[0]) and np.signbit(out[1])
    assert out[2] == np.inf and np.isnan(out[3]) and np.isnan(out[4])
    assert out[5] == np.float32(1e-45)                              # 1 denormal step * 0.75 -> 1 step, + 0.25 step -> rounds back to 1
    assert out[6] == pytest.approx(3e38, rel=1e-6) and out[7] == pytest.approx(1.5e38, rel=1e-6)      # no overflow on the way
    assert E.same_bits(E.update(ema, src, 0.0)[[0, 1, 5, 6]], ema[[0, 1, 5, 6]])
    assert np.isnan(E.update(ema, src, 0.0)[3]) and np.isnan(E.update(ema, src, 1.0)[2])       # inf * 0


@pytest.mark.parametrize("c", [0.0002, 0.5, E.coefficient("ExpMomentumEMA", 0.0002, 2000, 1)])
def test_torch_cpu_mul_add_is_within_one_ulp_of_the_restatement(c):
    """The restatement, not torch's CPU kernel, is the bit-exact yardstick: whether `add_(alpha=)` fuses depends on how torch was
    built for the host.  Either way the two stay within one ulp WHERE AVERAGE AND WEIGHT HAVE THE SAME SIGN (an average and the
    weight it follows): unfused, the product src * c is rounded too, by at most half an ulp of a term that is no larger than the
    sum, on top of the sum's own half ulp.  (With opposite signs the sum can cancel and the product's rounding error grows without
    bound in ulps of the result -- which is why the kernel's order is stated and the restatement is the yardstick.)"""
    g = torch.Generator().manual_seed(11)
    ema = torch.randn(4096, generator=g)
    ema = torch.where(ema.abs() < 1e-6, torch.full_like(ema, 1e-6), ema)
    src = ema * (1 + 0.01 * torch.randn(4096, generator=g).clamp(-50, 50))
    assert bool((torch.sign(src) == torch.sign(ema)).all())
    want = E.update(ema.numpy(), src.numpy(), c)
    got = ema.clone().mul_(1 - c).add_(src, alpha=c).numpy()
    d = E.ulp_distance(got, want)
    print(f"\nc={c:.6g}: torch CPU mul_/add_ equals the restatement bit for bit in {float((d == 0).mean()):.4f} of 4096, max {int(d.max())} ulp")
    assert int(d.max()) <= 1
