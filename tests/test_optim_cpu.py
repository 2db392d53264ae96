"""CPU: ``waldo_amd.optim`` without a GPU -- the framework-op route of ``optim.Adam`` / ``AdamW`` and the tests' own
restatement (``optim_ref``) against ``torch.optim.Adam`` / ``AdamW`` (``foreach=False``) in fp64, the clip against
``clip_grad_norm_``, the skip and the scale rule, state interchange with ``torch.optim.Adam``, ``from_opt``'s groups and
the refusals."""
import copy
import types

import pytest
import torch

import optim_ref as R

SIZES = [(3, 5), (7,), (1,), (4, 2, 3), (0,), (33,)]
DECAYS = [0.1, 0.0, 0.0, 0.05, 0.1, 0.0]
STEPS = 4
# fp64 rounding: a few ulps of values of order 1
RTOL, ATOL = 1e-12, 1e-14


def same(a, b):
    return torch.allclose(a, b, rtol=RTOL, atol=ATOL)


def make(dtype=torch.float64, seed=0):
    g = torch.Generator().manual_seed(seed)
    params = [torch.randn(s, generator=g, dtype=dtype) for s in SIZES]
    grads = [[torch.randn(s, generator=g, dtype=dtype) * 10.0 ** float(torch.randint(-3, 3, (1,), generator=g))
              for s in SIZES] for _ in range(STEPS)]
    return params, grads


def torch_run(params, grads, adamw, betas, max_norm, decays):
    ps = [torch.nn.Parameter(p.clone()) for p in params]
    groups = [dict(params=[p], weight_decay=wd if adamw else 0.0) for p, wd in zip(ps, decays)]
    cls = torch.optim.AdamW if adamw else torch.optim.Adam
    opt = cls(groups, lr=1e-2, betas=betas, eps=1e-8, foreach=False)
    out = []
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = g.clone()
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_(ps, max_norm, foreach=False)
        opt.step()
        out.append([p.detach().clone() for p in ps])
    return out, opt, ps


def ours_run(params, grads, adamw, betas, max_norm, decays, **kw):
    from waldo_amd import optim
    ps = [torch.nn.Parameter(p.clone()) for p in params]
    groups = [dict(params=[p], weight_decay=wd if adamw else 0.0) for p, wd in zip(ps, decays)]
    opt = (optim.AdamW if adamw else optim.Adam)(groups, lr=1e-2, betas=betas, eps=1e-8, max_norm=max_norm, **kw)
    out = []
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = g.clone()
        opt.step()
        out.append([p.detach().clone() for p in ps])
    return out, opt, ps


@pytest.mark.parametrize("max_norm", [0.0, 0.5])
@pytest.mark.parametrize("adamw,betas", [(False, (0.0, 0.99)), (False, (0.9, 0.999)), (True, (0.9, 0.99))])
def test_restatement_and_cpu_route_agree_with_torch_in_fp64(adamw, betas, max_norm):
    params, grads = make()
    want, topt, tps = torch_run(params, grads, adamw, betas, max_norm, DECAYS)
    got, opt, ps = ours_run(params, grads, adamw, betas, max_norm, DECAYS)
    ref = R.run(params, grads, dtype=torch.float64, lr=1e-2, betas=betas, eps=1e-8, max_norm=max_norm,
                weight_decays=DECAYS, adamw=adamw)
    for k in range(STEPS):
        for i in range(len(SIZES)):
            assert same(got[k][i], want[k][i]), (k, i)
            assert same(ref[k][0][i], want[k][i]), (k, i)
    assert not same(want[-1][0], params[0])                              # (and the parameters did move)
    for i, p in enumerate(tps):
        if p.numel():
            assert same(opt.state[ps[i]]["exp_avg"], topt.state[p]["exp_avg"]), i
            assert same(opt.state[ps[i]]["exp_avg_sq"], topt.state[p]["exp_avg_sq"]), i
            assert same(ref[-1][1][i], topt.state[p]["exp_avg"]) and same(ref[-1][2][i], topt.state[p]["exp_avg_sq"]), i
    assert float(opt.step_count) == STEPS and float(opt.skipped) == 0
    if max_norm > 0:   # the norm clip_grad_norm_ saw at the last step, and a coefficient that did clip
        norm = torch.sqrt(sum(g.square().sum() for g in grads[-1]))
        assert same(opt.grad_norm, norm) and float(opt.clip_coef) < 1
        assert abs(ref[-1][3]["grad_norm"] - float(norm)) <= 1e-12 * float(norm)
    else:
        assert float(opt.clip_coef) == 1


def test_fp32_cpu_route_follows_the_restatement():
    params, grads = make(torch.float32)
    got, _, _ = ours_run(params, grads, True, (0.9, 0.99), 0.5, DECAYS)
    ref = R.run(params, grads, dtype=torch.float32, lr=1e-2, betas=(0.9, 0.99), eps=1e-8, max_norm=0.5,
                weight_decays=DECAYS, adamw=True)
    for i in range(len(SIZES)):
        assert got[-1][i].dtype == torch.float32
        assert torch.allclose(got[-1][i], ref[-1][0][i], rtol=1e-5, atol=1e-6), i


@pytest.mark.parametrize("how", ["nan_grad", "inf_grad", "nan_loss"])
def test_a_non_finite_step_changes_nothing_and_is_counted(how):
    params, grads = make()
    bad = [g.clone() for g in grads[1]]
    loss = torch.tensor(1.0, dtype=torch.float64)
    if how == "nan_grad":
        bad[-1][-1] = float("nan")
    elif how == "inf_grad":
        bad[0][0, 0] = float("-inf")
    else:
        loss = torch.tensor(float("nan"), dtype=torch.float64)
    seq = [grads[0], bad, grads[2]]
    from waldo_amd import optim
    ps = [torch.nn.Parameter(p.clone()) for p in params]
    opt = optim.Adam(ps, lr=1e-2)
    twin, _, tps = ours_run(params, [grads[0], grads[2]], False, (0.0, 0.99), 0.0, DECAYS)
    for k, gs in enumerate(seq):
        for p, g in zip(ps, gs):
            p.grad = g.clone()
        before = [p.detach().clone() for p in ps], copy.deepcopy({i: opt.state[p] for i, p in enumerate(ps) if p in opt.state})
        opt.step(loss if k == 1 else None)
        if k == 1:
            for i, p in enumerate(ps):
                assert torch.equal(p.detach(), before[0][i]), i
                for key in ("exp_avg", "exp_avg_sq"):
                    assert torch.equal(opt.state[p][key], before[1][i][key]), (i, key)
            assert float(opt.step_count) == 1 and float(opt.skipped) == 1 and float(opt.skipped_in_a_row) == 1
    for i, p in enumerate(ps):
        assert torch.equal(p.detach(), twin[-1][i]), i
    assert float(opt.step_count) == 2 and float(opt.skipped) == 1 and float(opt.skipped_in_a_row) == 0
    # the restatement skips the same way
    ref = R.run(params, seq, dtype=torch.float64, lr=1e-2, betas=(0.0, 0.99), eps=1e-8)
    if how != "nan_loss":
        assert ref[1][3]["skipped"] == 1 and ref[1][3]["step"] == 1 and ref[2][3]["skipped_in_a_row"] == 0
        for i in range(len(SIZES)):
            assert torch.equal(ref[1][0][i], ref[0][0][i]) and same(ref[2][0][i], twin[-1][i]), i


def test_scale_backs_off_and_grows():
    from waldo_amd import optim
    p = torch.nn.Parameter(torch.ones(5, dtype=torch.float64))
    opt = optim.Adam([p], scaler=R.SCALER)
    st = R.new_state(R.SCALER["init_scale"])
    rp, rm, rv = [torch.ones(5, dtype=torch.float64)], [torch.zeros(5, dtype=torch.float64)], [torch.zeros(5, dtype=torch.float64)]
    assert float(opt.loss_scale) == 1024.0
    assert float(opt.scale(torch.tensor(2.0, dtype=torch.float64))) == 2048.0
    for bad, want in zip(R.SCALE_STEPS_BAD, R.SCALE_AFTER):
        g = torch.full((5,), float("inf") if bad else 0.25, dtype=torch.float64) * float(opt.loss_scale)
        p.grad = g.clone()
        opt.step()
        R.step(rp, [g], rm, rv, st, lr=1e-4, betas=(0.0, 0.99), eps=1e-8,
               **{k: v for k, v in R.SCALER.items() if k != "init_scale"})
        assert float(opt.loss_scale) == want == st["scale"], (bad, want, float(opt.loss_scale), st["scale"])
    assert float(opt.skipped) == sum(R.SCALE_STEPS_BAD) and same(p.detach(), rp[0])
    # the scaled gradients gave the unscaled run's update
    q = torch.nn.Parameter(torch.ones(5, dtype=torch.float64))
    plain = optim.Adam([q])
    for bad in R.SCALE_STEPS_BAD:
        if not bad:
            q.grad = torch.full((5,), 0.25, dtype=torch.float64)
            plain.step()
    assert same(p.detach(), q.detach())


def test_state_round_trips_through_torch_adam():
    from waldo_amd import optim
    params, grads = make()
    want, _, _ = torch_run(params, grads, False, (0.9, 0.99), 0.0, DECAYS)
    # ours for two steps, torch for the rest
    _, opt, ps = ours_run(params, grads[:2], False, (0.9, 0.99), 0.0, DECAYS)
    sd = opt.state_dict()
    assert all(set(v) == {"step", "exp_avg", "exp_avg_sq"} and float(v["step"]) == 2 for v in sd["state"].values())
    tps = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    topt = torch.optim.Adam([dict(params=[p]) for p in tps], lr=1e-2, betas=(0.9, 0.99), eps=1e-8, foreach=False)
    topt.load_state_dict(sd)
    for gs in grads[2:]:
        for p, g in zip(tps, gs):
            p.grad = g.clone()
        topt.step()
    for i, p in enumerate(tps):
        assert same(p.detach(), want[-1][i]), i
    # torch for two steps, ours for the rest
    _, topt, tps = torch_run(params, grads[:2], False, (0.9, 0.99), 0.0, DECAYS)
    ps = [torch.nn.Parameter(p.detach().clone()) for p in tps]
    opt = optim.Adam([dict(params=[p]) for p in ps], lr=1e-3, betas=(0.5, 0.5), max_norm=7.0)
    opt.load_state_dict(topt.state_dict())
    assert float(opt.step_count) == 2
    assert float(opt.hyper[optim.HY_LR]) == 1e-2 and float(opt.hyper[optim.HY_BETA1]) == 0.9    # the groups' values
    assert float(opt.hyper[optim.HY_MAX_NORM]) == 7.0                                           # torch has none: kept
    opt.hyper[optim.HY_MAX_NORM] = 0.0
    for gs in grads[2:]:
        for p, g in zip(ps, gs):
            p.grad = g.clone()
        opt.step()
    for i, p in enumerate(ps):
        assert same(p.detach(), want[-1][i]), i
    # and through its own dict
    again = optim.Adam([dict(params=[torch.nn.Parameter(p.detach().clone())]) for p in ps], lr=1e-2, betas=(0.9, 0.99))
    again.load_state_dict(opt.state_dict())
    assert float(again.step_count) == STEPS
    for a, b in zip(again.state.values(), opt.state.values()):
        assert torch.equal(a["exp_avg"], b["exp_avg"]) and torch.equal(a["exp_avg_sq"], b["exp_avg_sq"])


def test_parameters_without_a_gradient_are_left_out():
    from waldo_amd import optim
    a, b = torch.nn.Parameter(torch.ones(3, dtype=torch.float64)), torch.nn.Parameter(torch.ones(3, dtype=torch.float64))
    opt = optim.Adam([a, b], lr=1e-2)
    assert opt.step() is None and float(opt.step_count) == 0          # no gradient anywhere: nothing happens
    a.grad = torch.ones(3, dtype=torch.float64)
    opt.step()
    assert torch.equal(b.detach(), torch.ones(3, dtype=torch.float64)) and b not in opt.state
    assert not torch.equal(a.detach(), torch.ones(3, dtype=torch.float64)) and float(opt.step_count) == 1


class _Net(torch.nn.Module):
    def __init__(self, split):
        super().__init__()
        self.lin = torch.nn.Linear(4, 3)
        self.norm = torch.nn.LayerNorm(3)
        self.pos_embed = torch.nn.Parameter(torch.zeros(1, 2, 3))
        self.frozen = torch.nn.Parameter(torch.zeros(2, 2), requires_grad=False)
        if split:
            self.no_weight_decay = lambda: {"pos_embed"}


def test_from_opt_builds_the_reference_optimizers():
    from waldo_amd import optim
    o = types.SimpleNamespace(optimizer="adam", lr=2e-4, beta1=0.5, beta2=0.9, wd=0.01, clip_value=1.5)
    net = _Net(split=True)
    adam = optim.from_opt(net, o)
    assert type(adam) is optim.Adam and len(adam.param_groups) == 1
    g = adam.param_groups[0]
    assert (g["lr"], g["betas"], g["weight_decay"], g["max_norm"]) == (2e-4, (0.5, 0.9), 0, 1.5)   # wd is ignored, as there
    assert len(g["params"]) == len(list(net.parameters()))
    assert torch.allclose(adam.hyper[:5], torch.tensor([2e-4, 0.5, 0.9, 1e-8, 1.5]))
    o.optimizer = "adamw"
    split = optim.from_opt(net, o)
    assert type(split) is optim.AdamW and [g["weight_decay"] for g in split.param_groups] == [0.0, 0.01]
    no_decay, decay = (set(map(id, g["params"])) for g in split.param_groups)
    assert no_decay == {id(net.lin.bias), id(net.norm.weight), id(net.norm.bias), id(net.pos_embed)}
    assert decay == {id(net.lin.weight)}                                   # the frozen one is in neither
    whole = optim.from_opt(_Net(split=False), o)
    assert len(whole.param_groups) == 1 and whole.param_groups[0]["weight_decay"] == 0.01
    assert len(whole.param_groups[0]["params"]) == 6           # net.parameters(), the frozen one too: as there
    assert optim.from_opt(None, o) is None and optim.from_opt(torch.nn.Identity(), o) is None
    o.use_amp = True
    assert float(optim.from_opt(net, o).loss_scale) == 65536.0
    o.optimizer = "sgd"
    with pytest.raises(ValueError, match="adamw"):
        optim.from_opt(net, o)
    # the defaults are the reference's
    d = optim.Adam(net.parameters()).param_groups[0]
    assert (d["lr"], d["betas"], d["eps"], d["weight_decay"], d["max_norm"]) == (1e-4, (0.0, 0.99), 1e-8, 0, 0)


def test_refusals():
    from waldo_amd import optim
    from waldo_amd._lib import WaldoHipError
    from waldo_amd.tools.lvd_step import LvdStep
    from waldo_amd.tools.wif_step import WifStep
    p = torch.nn.Parameter(torch.ones(3))
    for kw in (dict(amsgrad=True), dict(maximize=True), dict(weight_decay=0.1), dict(scaler=dict(init=2.0)),
               dict(betas=(1.0, 0.9))):
        with pytest.raises(ValueError):
            optim.Adam([p], **kw)
    with pytest.raises(ValueError, match="shared"):
        optim.AdamW([dict(params=[p], lr=1e-3), dict(params=[torch.nn.Parameter(torch.ones(2))])])
    for dt in (torch.float16, torch.bfloat16):
        with pytest.raises(WaldoHipError, match="16-bit"):
            optim.Adam([torch.nn.Parameter(torch.ones(3, dtype=dt))])
        x = torch.ones(3, dtype=dt)
        with pytest.raises(WaldoHipError, match="16-bit"):
            optim.adam_step_([x], [x], [x], [x], optim.new_state("cpu"), optim.new_hyper("cpu"))
    x = torch.ones(4)
    st, hy = optim.new_state("cpu"), optim.new_hyper("cpu")
    with pytest.raises(ValueError, match="one length"):
        optim.adam_step_([x], [x, x], [x], [x], st, hy)
    with pytest.raises(ValueError, match="contiguous"):
        optim.adam_step_([torch.ones(4, 4).t()], [torch.ones(4, 4)], [torch.ones(4, 4)], [torch.ones(4, 4)], st, hy)
    with pytest.raises(ValueError, match="L2"):
        optim.adam_step_([x], [x], [x], [x], st, hy, weight_decays=[0.1])
    with pytest.raises(ValueError, match="one element"):
        optim.adam_step_([x], [x], [x], [x], st, hy, loss=torch.ones(2))
    with pytest.raises(ValueError, match="nets='reference'"):
        LvdStep(1, torch.device("cpu"), optimizer="adam")
    with pytest.raises(ValueError, match="unet='reference'"):
        WifStep(1, torch.device("cpu"), optimizer="adam")
    with pytest.raises(ValueError, match="optimizer must be"):
        optim.resolve("sgd", [p], "FlpStep")
