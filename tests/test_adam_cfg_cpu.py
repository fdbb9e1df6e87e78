"""CPU: the optimizer's own dict on the host (erd_amd/optim_cfg.py check_optimizer), AdamW's / Adam's bias corrections, the
param_groups a checkpoint stores under AdamW, and the AdamW example config."""
import os

import pytest
import torch

from erd_amd import Config, MODELS
from erd_amd import optim_cfg as OC
from e2e_util import CFG_INCRE, ROOT

CFG_ADAMW = os.path.join(ROOT, "configs", "gfl_increment", "gfl_r50_fpn_1x_coco_first_40_incre_last_40_cats_adamw.py")


def test_check_optimizer_accepts_sgd_adamw_adam_and_rejects_the_rest():
    sgd = dict(type="SGD", lr=0.01, momentum=0.9, weight_decay=1e-4, nesterov=True)
    assert OC.check_optimizer(sgd) == sgd                           # SGD passes as it is (nesterov is ignored as before)
    assert OC.check_optimizer(None) == dict(type="SGD")
    assert OC.check_optimizer(Config.fromfile(CFG_INCRE).optim_wrapper.optimizer) == dict(type="SGD", lr=0.01, momentum=0.9,
                                                                                         weight_decay=0.0001)
    got = OC.check_optimizer(dict(type="AdamW", lr=1e-4, betas=[0.9, 0.999], weight_decay=0.05))
    assert got == dict(type="AdamW", lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05) and isinstance(got["betas"], tuple)
    # torch's defaults: decoupled decay 0.01 for AdamW, none for Adam
    assert OC.check_optimizer(dict(type="AdamW")) == dict(type="AdamW", lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    assert OC.check_optimizer(dict(type="Adam", eps=1e-3, amsgrad=False, maximize=False)) == dict(
        type="Adam", lr=1e-3, betas=(0.9, 0.999), eps=1e-3, weight_decay=0.0)
    for bad in (dict(type="AdamW", amsgrad=True), dict(type="Adam", maximize=True), dict(type="RMSprop", lr=0.01),
                dict(type="Lion"), dict(lr=0.01)):
        with pytest.raises(NotImplementedError):
            OC.check_optimizer(bad)
    with pytest.raises(ValueError, match="momentum"):
        OC.check_optimizer(dict(type="AdamW", lr=1e-4, momentum=0.9))
    with pytest.raises(ValueError, match="fused"):
        OC.check_optimizer(dict(type="Adam", fused=True))
    for betas in ((1.0, 0.999), (0.9, 1.0), (-0.1, 0.999), (0.9, 1.5), (0.9,), 0.9):
        with pytest.raises(ValueError, match="betas"):
            OC.check_optimizer(dict(type="AdamW", betas=betas))
    assert OC.check_optimizer(dict(type="Adam", betas=(0.0, 0.0)))["betas"] == (0.0, 0.0)


@pytest.mark.parametrize("t", [1, 2, 1000])
def test_bias_corrections_are_those_of_torch_in_double(t):
    b1, b2 = 0.9, 0.999
    inv1, inv_sqrt2 = OC.adam_bias_corrections(b1, b2, t)
    assert inv1 == 1.0 / (1 - b1 ** t) and inv_sqrt2 == 1.0 / (1 - b2 ** t) ** 0.5
    # ... which is what one host step divides by: from zero state exp_avg = (1 - b1) g, exp_avg_sq = (1 - b2) g^2 at step t
    p = torch.nn.Parameter(torch.tensor([2.0], dtype=torch.float64))
    opt = torch.optim.Adam([p], lr=0.5, betas=(b1, b2), eps=0.0)
    opt.state[p] = dict(step=torch.tensor(float(t - 1)), exp_avg=torch.zeros(1, dtype=torch.float64),
                        exp_avg_sq=torch.zeros(1, dtype=torch.float64))
    p.grad = torch.tensor([3.0], dtype=torch.float64)
    opt.step()
    want = 2.0 - 0.5 * inv1 * ((1 - b1) * 3.0) / ((1 - b2) ** 0.5 * 3.0 * inv_sqrt2)
    assert float(p.detach()) == pytest.approx(want, rel=1e-14)
    with pytest.raises(ValueError):
        OC.adam_bias_corrections(b1, b2, 0)


@pytest.mark.parametrize("paramwise", [None, dict(norm_decay_mult=0., custom_keys={'backbone': dict(lr_mult=0.1)})])
def test_adamw_param_groups_load_into_torch_adamw_and_step(paramwise):
    cfg = Config.fromfile(CFG_INCRE)
    cfg.model.latest_model_flag = False
    model = MODELS.build(cfg.model)
    names = [n for n, _ in model.named_parameters()]
    opt_cfg = OC.check_optimizer(dict(type="AdamW", lr=1e-4, betas=(0.9, 0.999), weight_decay=0.05))
    if paramwise is None:
        groups = [OC.adam_param_group(opt_cfg, 1e-5, 1e-4, 0.05, list(range(len(names))))]
    else:
        rows = OC.resolve_paramwise(model, 1e-4, 0.05, paramwise)
        groups = OC.build_param_groups(rows, last_lr=1e-5, base_lr=1e-4, momentum=0.9, optimizer=opt_cfg)
        assert len(groups) == len(names) and [g["params"] for g in groups] == [[i] for i in range(len(names))]
        g = groups[names.index("backbone.layer2.0.conv1.weight")]
        assert g["lr"] == pytest.approx(1e-6, rel=1e-12) and g["initial_lr"] == pytest.approx(1e-5, rel=1e-12) and g["weight_decay"] == 0.05
        g = groups[names.index("bbox_head.cls_convs.0.gn.weight")]
        assert g["lr"] == pytest.approx(1e-5, rel=1e-12) and g["weight_decay"] == 0.0
        # the SGD layout is what it was
        sgd = OC.build_param_groups(rows, 1e-5, 1e-4, 0.9)
        assert sgd == OC.build_param_groups(rows, 1e-5, 1e-4, 0.9, optimizer=dict(type="SGD"))
        assert set(sgd[0]) == {"lr", "momentum", "dampening", "weight_decay", "nesterov", "maximize", "foreach", "differentiable",
                               "initial_lr", "params"}
    for g in groups:
        assert {"lr", "betas", "eps", "weight_decay", "amsgrad", "maximize", "foreach", "capturable", "differentiable", "fused",
                "initial_lr", "params"} <= set(g)
        assert g["betas"] == (0.9, 0.999) and g["eps"] == 1e-8 and g["amsgrad"] is False and g["maximize"] is False
    ps = [torch.nn.Parameter(torch.ones(2)) for _ in names]
    opt = torch.optim.AdamW([dict(params=[p]) for p in ps] if paramwise is not None else ps, lr=1.0)
    i = names.index("bbox_head.gfl_cls.weight")
    state = {i: dict(step=torch.tensor(3.0), exp_avg=torch.full((2,), 0.5), exp_avg_sq=torch.full((2,), 0.25))}
    opt.load_state_dict(dict(state=state, param_groups=groups))
    assert opt.param_groups[-1]["lr"] == 1e-5 and opt.param_groups[-1]["weight_decay"] == 0.05
    ps[i].grad = torch.ones(2)
    opt.step()
    assert float(opt.state[ps[i]]["step"]) == 4.0 and float(ps[i][0]) < 1.0
    assert torch.allclose(opt.state[ps[i]]["exp_avg"], torch.full((2,), 0.55))


def test_adamw_config_loads_without_leftover_sgd_keys():
    cfg = Config.fromfile(CFG_ADAMW)
    ow = cfg.optim_wrapper
    assert ow.optimizer.to_dict() == dict(type="AdamW", lr=1e-4, betas=(0.9, 0.999), weight_decay=0.05) or \
        ow.optimizer.to_dict() == dict(type="AdamW", lr=1e-4, betas=[0.9, 0.999], weight_decay=0.05)
    assert "momentum" not in ow.optimizer and "_delete_" not in ow.optimizer and ow.type == "OptimWrapper"
    assert OC.check_optimizer(ow.optimizer) == dict(type="AdamW", lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
    assert ow.paramwise_cfg.to_dict() == dict(norm_decay_mult=0., custom_keys={'backbone': dict(lr_mult=0.1)})
    assert ow.clip_grad == dict(max_norm=35, norm_type=2) and ow.get("accumulative_counts") is None
    assert cfg.model.type == "GFLIncrementERD" and cfg.train_dataloader.dataset.ann_file.endswith("sel_last_40_cats.json")
    assert cfg.param_scheduler[0].type == "LinearLR" and cfg.auto_scale_lr == dict(enable=True, base_batch_size=16)
    import inspect
    from erd_amd.engine import ERDTrainer
    assert list(inspect.signature(ERDTrainer.__init__).parameters)[-1] == "optimizer"
