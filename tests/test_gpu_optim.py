"""GPU: the optimizer step's kernels (include/waldo_hip.h "Optimizer step") through ``optim.adam_step_``, the functional
form, against ``optim_ref`` on the CPU in fp32 and fp64 fed the same fp32 gradients -- parity of the cumulative update and
of both moments over four steps, the clip, the skip, the loss scale, no host read, determinism -- and ``optim.Adam``'s
state moving to ``torch.optim.Adam`` and back.

The tensor list: sizes 0, 1, 3, 4, 5, 1023, one chunk, one chunk -+ 1, two chunks + 1, K + 1 tensors of two elements (more
than one launch per phase), a view that starts one element into a larger buffer (every base only 4-byte aligned) and a
tensor of which only the parameter is such a view.  Gradient magnitudes span 1e-12 .. 1e3 with exact zeros; lr = 1e-2, so
that an update is far above parity.TOL times the parameters' scale."""
import pytest
import torch

import optim_ref as R
from parity import close

pytestmark = pytest.mark.gpu
LR, EPS, STEPS = 1e-2, 1e-8, 4


def geometry():
    from waldo_amd import optim
    lim = optim.limits()
    return lim["tensors_per_launch"], lim["chunk"]


def sizes():
    k, chunk = geometry()
    return [0, 1, 3, 4, 5, 1023, chunk, chunk - 1, chunk + 1, 2 * chunk + 1] + [2] * (k + 1)


N_VIEWS = 2   # the two tensors after sizes(): all four buffers offset by one element; only the parameter offset


def view_size():
    return geometry()[1] + 5   # two chunks on the element path, numel % 4 == 1


def make_grads(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for n in shapes:
        mag = 10.0 ** (torch.rand(n, generator=g) * 15 - 12)                      # 1e-12 .. 1e3
        sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
        x = (mag * sign).float()
        x[torch.rand(n, generator=g) < 0.1] = 0.0                                 # exact zeros
        out.append(x)
    return out


@pytest.fixture(scope="module")
def problem():
    """CPU fp32: the initial parameters, the gradients of each step and the per-tensor decays."""
    shapes = sizes() + [view_size()] * N_VIEWS
    g = torch.Generator().manual_seed(1)
    params = [0.5 * torch.randn(n, generator=g) for n in shapes]
    grads = [make_grads(shapes, 10 + s) for s in range(STEPS)]
    decays = [0.1 if i % 2 == 0 else 0.0 for i in range(len(shapes))]
    return dict(shapes=shapes, params=params, grads=grads, decays=decays)


class Run:
    """The lists of one optimizer on the device, in the problem's layout (the last N_VIEWS tensors are views), stepped
    through ``optim.adam_step_``."""

    def __init__(self, problem, dev, *, adamw=False, betas=(0.0, 0.99), max_norm=0.0, scaler=False, lr=LR):
        from waldo_amd import optim
        self.dev, self.adamw = dev, adamw
        self.decays = problem["decays"] if adamw else None
        n = len(problem["shapes"])

        def place(t, offset):
            if not offset:
                return t.to(dev).clone()
            buf = torch.zeros(t.numel() + 8, device=dev)
            v = buf[1:1 + t.numel()]
            v.copy_(t)
            assert v.data_ptr() % 16 == 4 and v.is_contiguous()
            return v
        self.off_all = [i == n - 2 for i in range(n)]     # p, g, m, v one element in
        self.off_p = [i >= n - 2 for i in range(n)]       # the last one: only p (g, m, v are aligned)
        self.p = [place(t, o) for t, o in zip(problem["params"], self.off_p)]
        self.m = [place(torch.zeros_like(t), o) for t, o in zip(problem["params"], self.off_all)]
        self.v = [place(torch.zeros_like(t), o) for t, o in zip(problem["params"], self.off_all)]
        self.state = optim.new_state(dev)
        self.hyper = optim.new_hyper(dev, lr, betas, EPS, max_norm, scaler)
        self.launches = None

    def grads(self, cpu_grads, mul=1.0):
        return [self._g(t * mul, o) for t, o in zip(cpu_grads, self.off_all)]

    def _g(self, t, offset):
        if not offset:
            return t.to(self.dev)
        buf = torch.zeros(t.numel() + 8, device=self.dev)
        buf[1:1 + t.numel()].copy_(t)
        return buf[1:1 + t.numel()]

    def step(self, grads, loss=None):
        from waldo_amd import optim
        self.launches = optim.adam_step_(self.p, grads, self.m, self.v, self.state, self.hyper, weight_decays=self.decays,
                                         adamw=self.adamw, loss=loss)

    def word(self, i):
        return float(self.state[i])

    def clone(self):
        return [x.clone() for x in self.p], [x.clone() for x in self.m], [x.clone() for x in self.v], self.state.clone()


CONFIGS = {"adam": dict(adamw=False, betas=(0.0, 0.99)), "adamw": dict(adamw=True, betas=(0.9, 0.999))}
_REFS = {}


def reference(problem, name, dtype, **kw):
    """``optim_ref.run`` of the problem, computed once per configuration and shared."""
    key = (name, dtype, tuple(sorted(kw.items())))
    if key not in _REFS:
        cfg = CONFIGS[name]
        _REFS[key] = R.run(problem["params"], problem["grads"], dtype=dtype, lr=LR, betas=cfg["betas"], eps=EPS,
                           adamw=cfg["adamw"], weight_decays=problem["decays"] if cfg["adamw"] else None, **kw)
    return _REFS[key]


def compare_step(run, problem, r32, r64, k, what):
    p0 = problem["params"]
    for i, n in enumerate(problem["shapes"]):
        if n == 0:
            continue
        tag = f"{what} step {k} tensor {i} (n={n})"
        close(run.p[i].cpu() - p0[i], r32[k][0][i] - p0[i], rel=True, exact=r64[k][0][i] - p0[i].double(), what=tag + " update")
        close(run.m[i], r32[k][1][i], rel=True, exact=r64[k][1][i], what=tag + " exp_avg")
        close(run.v[i], r32[k][2][i], rel=True, exact=r64[k][2][i], what=tag + " exp_avg_sq")


@pytest.mark.parametrize("name", list(CONFIGS))
def test_parity_of_update_and_moments_over_four_steps(problem, dev, name):
    from waldo_amd import optim
    r32, r64 = reference(problem, name, torch.float32), reference(problem, name, torch.float64)
    run = Run(problem, dev, **CONFIGS[name])
    for k in range(STEPS):
        run.step(run.grads(problem["grads"][k]))
        compare_step(run, problem, r32, r64, k, name)
        if k == 0:   # every parameter with a non-zero gradient has moved
            for i, g in enumerate(problem["grads"][0]):
                moved = run.p[i].cpu() != problem["params"][i]
                assert bool(moved[g != 0].all()), (i, int((~moved[g != 0]).sum()))
                if not CONFIGS[name]["adamw"]:
                    assert not bool(moved[g == 0].any()), i
    assert run.word(optim.ST_STEP) == STEPS and run.word(optim.ST_SKIPPED) == 0 and run.word(optim.ST_FINITE) == 1
    assert run.word(optim.ST_COEF) == 1.0
    close(run.state[optim.ST_BC1].reshape(1), torch.tensor([1 - CONFIGS[name]["betas"][0] ** STEPS]), rel=True, what="bc1")
    close(run.state[optim.ST_SQRT_BC2].reshape(1), torch.tensor([(1 - CONFIGS[name]["betas"][1] ** STEPS) ** 0.5]), rel=True,
          what="sqrt bc2")


def test_clip(problem, dev):
    from waldo_amd import optim
    norm64 = [R.grad_norm([g.double() for g in gs]) for gs in problem["grads"]]
    norm32 = [R.grad_norm(gs) for gs in problem["grads"]]
    small = 0.5 * norm64[0]
    r32 = reference(problem, "adamw", torch.float32, max_norm=small)
    r64 = reference(problem, "adamw", torch.float64, max_norm=small)
    run = Run(problem, dev, max_norm=small, **CONFIGS["adamw"])
    for k in range(2):
        run.step(run.grads(problem["grads"][k]))
        close(run.state[optim.ST_NORM].reshape(1), torch.tensor([norm32[k]]), rel=True, exact=torch.tensor([norm64[k]], dtype=torch.float64),
              what=f"grad_norm step {k}")
        close(run.state[optim.ST_COEF].reshape(1), torch.tensor([r32[k][3]["clip_coef"]]), rel=True,
              exact=torch.tensor([r64[k][3]["clip_coef"]], dtype=torch.float64), what=f"clip_coef step {k}")
        assert run.word(optim.ST_COEF) < 1                                      # clipping is active
        compare_step(run, problem, r32, r64, k, "clipped")
    # max_norm above the norm: the coefficient clamps to exactly 1 -- and equals no clipping (max_norm = 0), bit for bit
    above, none = Run(problem, dev, max_norm=4.0 * max(norm64), **CONFIGS["adam"]), Run(problem, dev, **CONFIGS["adam"])
    for k in range(2):
        for r in (above, none):
            r.step(r.grads(problem["grads"][k]))
        assert above.word(optim.ST_COEF) == 1.0 == none.word(optim.ST_COEF)
        assert above.word(optim.ST_NORM) == none.word(optim.ST_NORM) > 0
    for a, b in zip(above.clone()[:3], none.clone()[:3]):
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def _poison(problem, how):
    """The gradients of step 1 with one bad element, and the loss of that step."""
    k, chunk = geometry()
    bad = [g.clone() for g in problem["grads"][1]]
    loss = torch.tensor(0.5)
    if how == "nan_last":                  # the last element of the last tensor
        bad[-1][-1] = float("nan")
    elif how == "inf_tail":                # a scalar tail: index numel - 1 where numel % 4 == 1 (one 16-byte group + 1)
        i = problem["shapes"].index(5)
        bad[i][4] = float("inf")
    elif how == "inf_tail_chunk":          # the same in a chunk of its own: one chunk + 1 elements
        i = problem["shapes"].index(chunk + 1)
        bad[i][chunk] = float("-inf")
    else:
        loss = torch.tensor(float("nan"))
    return bad, loss


@pytest.mark.parametrize("how", ["nan_last", "inf_tail", "inf_tail_chunk", "nan_loss"])
def test_a_non_finite_step_writes_nothing_and_the_next_is_a_twins(problem, dev, how):
    from waldo_amd import optim
    bad, loss = _poison(problem, how)
    run, twin = Run(problem, dev, **CONFIGS["adamw"]), Run(problem, dev, **CONFIGS["adamw"])
    for r in (run, twin):
        r.step(r.grads(problem["grads"][0]), loss=torch.tensor(0.5, device=dev))
    before = run.clone()
    run.step(run.grads(bad), loss=loss.to(dev))
    after = run.clone()
    for a, b in zip(before[:3], after[:3]):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert run.word(optim.ST_STEP) == 1 and run.word(optim.ST_SKIPPED) == 1 and run.word(optim.ST_SKIP_ROW) == 1
    assert run.word(optim.ST_FINITE) == 0
    for r in (run, twin):
        r.step(r.grads(problem["grads"][2]), loss=torch.tensor(0.25, device=dev))
    for a, b in zip(run.clone()[:3], twin.clone()[:3]):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert run.word(optim.ST_STEP) == 2 == twin.word(optim.ST_STEP)
    assert run.word(optim.ST_SKIP_ROW) == 0 and run.word(optim.ST_SKIPPED) == 1 and twin.word(optim.ST_SKIPPED) == 0


def test_scaled_gradients_give_the_unscaled_result(problem, dev):
    from waldo_amd import optim
    r32, r64 = reference(problem, "adam", torch.float32), reference(problem, "adam", torch.float64)
    run = Run(problem, dev, scaler=dict(init_scale=1024.0, growth_interval=1000), **CONFIGS["adam"])
    norm64 = R.grad_norm([g.double() for g in problem["grads"][0]])
    for k in range(2):
        run.step(run.grads(problem["grads"][k], mul=1024.0))
        compare_step(run, problem, r32, r64, k, "scaled")
        if k == 0:   # the norm is the unscaled one
            close(run.state[optim.ST_NORM].reshape(1), torch.tensor([norm64]), rel=True, what="unscaled norm")
    assert float(run.hyper[optim.HY_SCALE]) == 1024.0 and run.word(optim.ST_MULT) == 1 / 1024


def test_scale_backs_off_and_grows_as_on_the_cpu(dev):
    from waldo_amd import optim
    p, m, v = (torch.ones(5, device=dev) for _ in range(3))
    state, hyper = optim.new_state(dev), optim.new_hyper(dev, scaler=R.SCALER)
    got = []
    for bad in R.SCALE_STEPS_BAD:
        g = torch.full((5,), float("inf") if bad else 0.25, device=dev) * hyper[optim.HY_SCALE]
        optim.adam_step_([p], [g], [m], [v], state, hyper)
        got.append(float(hyper[optim.HY_SCALE]))
    assert tuple(got) == R.SCALE_AFTER
    assert float(state[optim.ST_SKIPPED]) == sum(R.SCALE_STEPS_BAD)
    assert float(state[optim.ST_STEP]) == len(R.SCALE_STEPS_BAD) - sum(R.SCALE_STEPS_BAD)


def test_a_step_reads_nothing_on_the_host_and_is_one_call_of_2n_plus_1_launches(problem, dev):
    from waldo_amd import _lib, optim
    k, _ = geometry()
    run, twin = Run(problem, dev, **CONFIGS["adamw"]), Run(problem, dev, **CONFIGS["adamw"])
    grads = [r.grads(problem["grads"][0]) for r in (run, twin)]
    loss = torch.tensor(0.5, device=dev)
    run.step(grads[0], loss=loss)    # (the library's first call is behind it)
    twin.step(grads[1], loss=loss)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with _lib.KernelTimer() as timer:
            run.step(grads[0], loss=loss)
        twin.step(grads[1], loss=loss)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    n = sum(1 for s in problem["shapes"] if s > 0)
    assert n > k                                                     # more than one launch per phase
    # ONE call of the library for the whole step, which launched 2 ceil(n / K) + 1 kernels (counted at its launch sites)
    assert {name: len(v) for name, v in timer.pairs.items()} == {"waldo_adam_step": 1}
    assert run.launches == 2 * ((n + k - 1) // k) + 1 == optim.launches_per_step(n)
    # the same inputs, the same bits
    for a, b in zip(run.clone(), twin.clone()):
        assert torch.equal(a, b) if torch.is_tensor(a) else all(torch.equal(x, y) for x, y in zip(a, b))


def _module(problem, dev):
    return [torch.nn.Parameter(t.to(dev).clone()) for t in problem["params"][:10]]


def _feed(ps, cpu_grads, dev):
    for p, g in zip(ps, cpu_grads):
        p.grad = g.to(dev)


def test_set_lr_takes_effect_without_a_sync(problem, dev):
    from waldo_amd import optim
    ps, qs = _module(problem, dev), _module(problem, dev)
    a, b = optim.Adam(ps, lr=LR), optim.Adam(qs, lr=0.5 * LR)
    for opt, leaves in ((a, ps), (b, qs)):
        _feed(leaves, problem["grads"][0], dev)
        opt.step()
    first_a, first_b = [p.detach().clone() for p in ps], [q.detach().clone() for q in qs]
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a.set_lr(0.5 * LR)
        for opt, leaves in ((a, ps), (b, qs)):
            for p in leaves:     # (the same gradient again: no copy from the host under the sync check)
                p.grad = p.grad.clone()
            opt.step(torch.zeros((), device=dev))
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert a.param_groups[0]["lr"] == 0.5 * LR and float(a.hyper[optim.HY_LR]) == float(b.hyper[optim.HY_LR])
    # the moments do not depend on lr: a's second step is b's second step, half of what lr = LR would have moved it
    for i in (1, 5, 6, 9):
        da, db = ps[i].detach() - first_a[i], qs[i].detach() - first_b[i]
        close(da, db, rel=True, what=f"second step after set_lr, tensor {i}")
        assert 0.25 * LR < float(da.abs().max()) < 0.75 * LR, (i, float(da.abs().max()))
        assert float((first_a[i] - problem["params"][i].to(dev)).abs().max()) > 0.75 * LR    # (the first moved by LR)
    assert float(a.step_count) == 2 and float(a.skipped) == 0


@pytest.mark.parametrize("direction", ["to_torch", "from_torch"])
def test_state_moves_between_this_optimizer_and_torch_adam(problem, dev, direction):
    """Two steps by one optimizer, its state_dict loaded into the other, two more steps: the four-step reference."""
    from waldo_amd import optim
    r32, r64 = reference(problem, "adamw", torch.float32), reference(problem, "adamw", torch.float64)
    betas = CONFIGS["adamw"]["betas"]
    decays = problem["decays"][:10]

    def build(cls, leaves, **kw):
        return cls([dict(params=[p], weight_decay=wd) for p, wd in zip(leaves, decays)], lr=LR, betas=betas, eps=EPS, **kw)
    ps = _module(problem, dev)
    ours, theirs = build(optim.AdamW, ps), build(torch.optim.AdamW, ps, foreach=False)
    first, second = (ours, theirs) if direction == "to_torch" else (theirs, ours)
    for k in range(2):
        _feed(ps, problem["grads"][k], dev)
        first.step()
    second.load_state_dict(first.state_dict())
    for k in range(2, 4):
        _feed(ps, problem["grads"][k], dev)
        second.step()
    for i, n in enumerate(problem["shapes"][:10]):
        if n:
            p0 = problem["params"][i]
            close(ps[i].detach().cpu() - p0, r32[3][0][i] - p0, rel=True, exact=r64[3][0][i] - p0.double(),
                  what=f"{direction} tensor {i} update")
            close(second.state[ps[i]]["exp_avg_sq"], r32[3][2][i], rel=True, exact=r64[3][2][i],
                  what=f"{direction} tensor {i} exp_avg_sq")
    if direction == "from_torch":
        assert float(ours.step_count) == 4


def test_the_kept_host_arrays_follow_the_set_of_gradients(dev):
    """``Adam.step`` keeps its host arrays between steps: a parameter that loses its gradient, one that gains one and a
    gradient that is not contiguous each take effect at the next step, as on the CPU route."""
    from waldo_amd import optim
    g = torch.Generator().manual_seed(5)
    init = [torch.randn(6, 5, generator=g), torch.randn(4097, generator=g), torch.randn(3, generator=g)]
    grads = [[torch.randn(t.shape, generator=g) for t in init] for _ in range(4)]
    have = [(0, 1), (0, 1), (1, 2), (1, 2)]          # which parameters have a gradient at each step
    results = []
    for device in (torch.device("cpu"), dev):
        ps = [torch.nn.Parameter(t.to(device).clone()) for t in init]
        opt = optim.AdamW([dict(params=ps[:2], weight_decay=0.1), dict(params=ps[2:], weight_decay=0.0)], lr=LR,
                          betas=(0.9, 0.99))
        for k, idx in enumerate(have):
            for i, p in enumerate(ps):
                p.grad = grads[k][i].to(device) if i in idx else None
            if k == 3:   # every other element of a buffer twice as long: the same values, not contiguous
                wide = torch.zeros(2 * init[1].numel(), device=device)
                wide[::2] = grads[k][1].to(device)
                ps[1].grad = wide[::2]
                assert not ps[1].grad.is_contiguous()
            opt.step()
        results.append(([p.detach().cpu() for p in ps], float(opt.step_count)))
    (cpu, n_cpu), (gpu, n_gpu) = results
    assert n_cpu == n_gpu == 4
    for i in range(3):
        close(gpu[i] - init[i], cpu[i] - init[i], rel=True, what=f"parameter {i} after four steps")
        assert not torch.equal(gpu[i], init[i])
