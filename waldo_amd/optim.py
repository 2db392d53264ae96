"""The optimizer step on the device (include/waldo_hip.h "Optimizer step"): what ends every training step of the reference
(models/synthesizer.py:1057-1072) -- the NaN test of the loss, ``GradScaler``'s unscale and update, ``clip_grad_norm_``
and ``torch.optim.Adam`` / ``AdamW`` -- as three phases of HIP kernels that read nothing on the host:

    opt = optim.Adam(net.parameters(), max_norm=1.0)        # or optim.from_opt(net, opt), optim.AdamW(...)
    loss = ...; opt.scale(loss).backward(); opt.step(loss)   # no sync; capturable in the step's graph
    opt.skipped, opt.grad_norm, opt.loss_scale               # device tensors: reading them is the caller's sync

The gradient norm, the clip coefficient, the skip decision, the bias corrections and the loss scale live in a small
``state`` vector in device memory, the hyper-parameters in a ``hyper`` vector next to it (``set_lr`` writes it without a
sync, also between the replays of a graph).  A step whose gradients hold a NaN or an inf, or whose ``loss`` is NaN, writes
nothing and is counted.  fp32 parameters on the GPU take the kernels; CPU tensors and fp64 take ``_framework_step``, the
same arithmetic in framework ops; 16-bit parameters are refused.  ``amsgrad``, ``maximize`` and L2-style decay
(``torch.optim.Adam``'s ``weight_decay``) are not offered.

One step counter serves every parameter: a parameter left out of steps for lack of a gradient is bias-corrected with the
optimizer's count, not its own (torch keeps one count per parameter).  Under DDP the all-reduced gradients carry a NaN to
every rank, so every rank skips the same steps; the reference's consensus on ``loss.isnan()`` (``engine.all_gather_tensor``)
is not restated.
"""
import ctypes

import torch

from . import _lib

STATE_WORDS, HYPER_WORDS = 16, 12
# include/waldo_hip.h: the words of `state` ...
ST_STEP, ST_NORM, ST_COEF, ST_MULT, ST_FINITE, ST_BC1, ST_SQRT_BC2, ST_STEP_SIZE, ST_SKIP_ROW, ST_SKIPPED, ST_GROWTH = range(11)
# ... and of `hyper`
HY_LR, HY_BETA1, HY_BETA2, HY_EPS, HY_MAX_NORM, HY_SCALE, HY_GROWTH_FACTOR, HY_BACKOFF_FACTOR, HY_GROWTH_INTERVAL = range(9)
# torch.cuda.amp.GradScaler's defaults (the reference builds it without arguments, models/synthesizer.py:146-152)
SCALER_DEFAULTS = dict(init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000)


def limits():
    """{"tensors_per_launch": K, "chunk": elements per workgroup, "state_words", "hyper_words"} of the library."""
    out = (ctypes.c_int * 4)()
    n = _lib.load().waldo_adam_limits(out, 4)
    assert n == 4, n
    return dict(zip(("tensors_per_launch", "chunk", "state_words", "hyper_words"), out))


def launches_per_step(n_tensors):
    """Kernel launches of one step over ``n_tensors`` non-empty tensors: 2 ceil(n / K) + 1."""
    k = limits()["tensors_per_launch"]
    return 2 * ((n_tensors + k - 1) // k) + 1


def new_state(device, dtype=torch.float32):
    return torch.zeros(STATE_WORDS, dtype=dtype, device=device)


def new_hyper(device, lr=1e-4, betas=(0.0, 0.99), eps=1e-8, max_norm=0.0, scaler=False, dtype=torch.float32):
    """The hyper vector.  ``scaler``: False (scale 1, never changed), True (``SCALER_DEFAULTS``) or a dict with any of
    init_scale, growth_factor, backoff_factor, growth_interval."""
    if scaler is False or scaler is None:
        s = dict(init_scale=1.0, growth_factor=1.0, backoff_factor=1.0, growth_interval=0)
    else:
        s = dict(SCALER_DEFAULTS)
        if scaler is not True:
            unknown = set(scaler) - set(s)
            if unknown:
                raise ValueError(f"optim: unknown scaler fields {sorted(unknown)}; known: {sorted(s)}")
            s.update(scaler)
        if not s["init_scale"] > 0 or not s["growth_factor"] >= 1 or not 0 < s["backoff_factor"] <= 1 \
                or s["growth_interval"] < 0:
            raise ValueError(f"optim: bad scaler constants {s}")
    if not lr >= 0 or not eps >= 0 or not 0 <= betas[0] < 1 or not 0 <= betas[1] < 1:
        raise ValueError(f"optim: bad hyper-parameters lr={lr} betas={betas} eps={eps}")
    words = [lr, betas[0], betas[1], eps, max_norm, s["init_scale"], s["growth_factor"], s["backoff_factor"],
             s["growth_interval"]]
    h = torch.zeros(HYPER_WORDS, dtype=torch.float64)
    h[:len(words)] = torch.tensor([float(w) for w in words], dtype=torch.float64)
    return h.to(dtype).to(device)


def _framework_step(params, grads, exp_avgs, exp_avg_sqs, state, hyper, weight_decays, adamw, loss):
    """The three phases in framework ops, in the parameters' dtype, with the scalars in fp64: the route of CPU tensors and
    of fp64.  Like the kernels it branches on nothing it has computed (the skip is a ``torch.where``)."""
    f64 = torch.float64
    dt = params[0].dtype
    h = hyper.to(f64)
    lr, b1, b2, eps, max_norm, scale = (h[i] for i in (HY_LR, HY_BETA1, HY_BETA2, HY_EPS, HY_MAX_NORM, HY_SCALE))
    growth, backoff, interval = h[HY_GROWTH_FACTOR], h[HY_BACKOFF_FACTOR], h[HY_GROWTH_INTERVAL]
    s = state.to(f64)
    total = torch.zeros((), dtype=f64, device=state.device)
    bad = torch.zeros((), dtype=torch.bool, device=state.device)
    for g in grads:
        if g.numel():
            total = total + g.to(f64).square().sum()
            bad = bad | ~torch.isfinite(g).all()
    if loss is not None:
        bad = bad | torch.isnan(loss).any()
    finite = ~bad
    norm = total.sqrt() / scale
    one = torch.ones((), dtype=f64, device=state.device)
    coef = torch.where(max_norm > 0, torch.clamp(max_norm / (norm + 1e-6), max=1.0), one)
    mult = coef / scale
    step = s[ST_STEP] + 1
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    step_size, sqrt_bc2 = lr / bc1, bc2.sqrt()
    for p, g, m, v, wd in zip(params, grads, exp_avgs, exp_avg_sqs, weight_decays):
        if p.numel() == 0:
            continue
        pn = p * (1 - lr * wd).to(dt) if adamw and wd != 0 else p
        gp = g * mult.to(dt)
        mn = torch.lerp(m, gp, (1 - b1).to(dt))
        vn = v * b2.to(dt) + ((1 - b2).to(dt) * gp) * gp
        pn = pn - step_size.to(dt) * (mn / (vn.sqrt() / sqrt_bc2.to(dt) + eps.to(dt)))
        p.copy_(torch.where(finite, pn, p))
        m.copy_(torch.where(finite, mn, m))
        v.copy_(torch.where(finite, vn, v))
    tracker = s[ST_GROWTH] + 1
    grow = finite & (interval > 0) & (tracker >= interval)
    zero = torch.zeros_like(one)
    new = s.clone()
    new[ST_NORM], new[ST_COEF], new[ST_MULT], new[ST_FINITE] = norm, coef, mult, finite.to(f64)
    for i, val in ((ST_STEP, step), (ST_BC1, bc1), (ST_SQRT_BC2, sqrt_bc2), (ST_STEP_SIZE, step_size),
                   (ST_SKIP_ROW, zero)):
        new[i] = torch.where(finite, val, s[i])
    new[ST_SKIP_ROW] = torch.where(finite, zero, s[ST_SKIP_ROW] + 1)
    new[ST_SKIPPED] = torch.where(finite, s[ST_SKIPPED], s[ST_SKIPPED] + 1)
    new[ST_GROWTH] = torch.where(bad | grow, zero, tracker)
    state.copy_(new.to(state.dtype))
    hyper[HY_SCALE] = torch.where(bad, scale * backoff, torch.where(grow, scale * growth, scale)).to(hyper.dtype)


def adam_step_(params, grads, exp_avgs, exp_avg_sqs, state, hyper, *, weight_decays=None, adamw=False, loss=None,
               workspace=None):
    """One step over the lists, in place: ``params``, ``exp_avgs``, ``exp_avg_sqs`` and ``state`` are updated, ``hyper``'s
    scale too.  Every tensor contiguous, of one dtype and device; ``state`` (``new_state``) and ``hyper`` (``new_hyper``)
    on that device.  ``weight_decays``: one float per tensor, used with ``adamw``.  ``loss``: a one-element tensor whose
    NaN skips the step.  ``workspace``: a uint8 buffer to use when it is large enough.  fp32 on the GPU: the kernels
    (returns the number of launches, 2 ceil(n / K) + 1 over n non-empty tensors); CPU tensors and fp64: framework ops
    (returns 0); 16-bit tensors: refused."""
    n = len(params)
    if not (len(grads) == len(exp_avgs) == len(exp_avg_sqs) == n):
        raise ValueError(f"adam_step_: the four lists must have one length, got {n}, {len(grads)}, {len(exp_avgs)}, "
                         f"{len(exp_avg_sqs)}")
    wds = [0.0] * n if weight_decays is None else [float(w) for w in weight_decays]
    if len(wds) != n:
        raise ValueError(f"adam_step_: {len(wds)} weight decays for {n} tensors")
    if any(w != 0 for w in wds) and not adamw:
        raise ValueError("adam_step_: a weight decay without adamw is torch.optim.Adam's L2 term, which is not offered")
    if state.numel() < STATE_WORDS or hyper.numel() < HYPER_WORDS or not state.is_contiguous() or not hyper.is_contiguous():
        raise ValueError(f"adam_step_: state needs {STATE_WORDS} and hyper {HYPER_WORDS} contiguous words")
    dev, dt = state.device, (params[0].dtype if n else state.dtype)
    for name, ts in (("params", params), ("grads", grads), ("exp_avgs", exp_avgs), ("exp_avg_sqs", exp_avg_sqs)):
        for i, t in enumerate(ts):
            if t.dtype in (torch.float16, torch.bfloat16):
                raise _lib.WaldoHipError(f"adam_step_: {name}[{i}] is {t.dtype}: 16-bit parameters are not supported "
                                         "(no master weights)")
            if t.dtype != dt or t.device != dev or not t.is_contiguous() or t.shape != params[i].shape:
                raise ValueError(f"adam_step_: {name}[{i}] must be a contiguous {dt} tensor on {dev} of shape "
                                 f"{tuple(params[i].shape)}, got {t.dtype} on {t.device}, shape {tuple(t.shape)}, "
                                 f"contiguous={t.is_contiguous()}")
    if loss is not None:
        if loss.numel() != 1 or loss.device != dev:
            raise ValueError(f"adam_step_: loss must be one element on {dev}, got {tuple(loss.shape)} on {loss.device}")
        loss = loss.detach()
    with torch.no_grad():
        if dev.type != "cuda" or dt == torch.float64:
            if dt not in (torch.float32, torch.float64) or hyper.dtype not in (torch.float32, torch.float64):
                raise ValueError(f"adam_step_: fp32 or fp64 tensors, got {dt} (hyper: {hyper.dtype})")
            _framework_step(params, grads, exp_avgs, exp_avg_sqs, state, hyper, wds, adamw, loss)
            return 0
        _lib.check_cuda(state, hyper, *params[:1])
        if loss is not None and loss.dtype != torch.float32:
            loss = loss.float()
        numels = (ctypes.c_int64 * n)(*[p.numel() for p in params])
        need = _lib.query("waldo_adam_workspace_bytes", n, numels)
        if need == 0:
            raise _lib.WaldoHipError("adam_step_: the tensors are too large for one step (more than 2^31 - 1 chunks)")
        if workspace is None or workspace.numel() * workspace.element_size() < need or workspace.device != dev:
            workspace = torch.empty(need, dtype=torch.uint8, device=dev)
        arrays = [(ctypes.c_void_p * n)(*[t.data_ptr() for t in ts]) for ts in (params, grads, exp_avgs, exp_avg_sqs)]
        return _launch(dev, arrays, numels, (ctypes.c_float * n)(*wds), n, state, hyper, loss, workspace, adamw)


def _launch(dev, arrays, numels, decays, n, state, hyper, loss, workspace, adamw):
    """``waldo_adam_step`` on checked arguments; returns the number of kernel launches."""
    launches = ctypes.c_int(0)
    with _lib.on_device(dev):
        _lib.call("waldo_adam_step", *arrays, numels, decays, n, state.data_ptr(), hyper.data_ptr(), _lib.ptr(loss),
                  workspace.data_ptr(), workspace.numel() * workspace.element_size(), int(bool(adamw)),
                  ctypes.byref(launches), _lib.current_stream(dev))
    return launches.value


class Adam(torch.optim.Optimizer):
    """``torch.optim.Adam`` with the clip (``max_norm``, the reference's ``clip_value``; 0: none), the NaN / inf skip and
    the loss scale (``scaler``: False, True or a dict, see ``new_hyper``) inside ``step``.  The defaults are the
    reference's (tools/options.py:583-589).  lr, betas and eps are the optimizer's, not a group's: only ``weight_decay``
    may differ between groups (``AdamW``)."""

    _adamw = False

    def __init__(self, params, lr=1e-4, betas=(0.0, 0.99), eps=1e-8, weight_decay=0, max_norm=0, scaler=False,
                 amsgrad=False, maximize=False):
        name = type(self).__name__
        if amsgrad or maximize:
            raise ValueError(f"{name}: amsgrad and maximize are not supported")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, max_norm=max_norm))
        first = self.param_groups[0]
        for g in self.param_groups:
            if any(g[k] != first[k] for k in ("lr", "betas", "eps", "max_norm")):
                raise ValueError(f"{name}: lr, betas, eps and max_norm are shared by all groups (one hyper vector); only "
                                 "weight_decay may differ")
            if g["weight_decay"] != 0 and not self._adamw:
                raise ValueError(f"{name}: weight_decay is torch.optim.Adam's L2 term, which is not supported: use AdamW "
                                 "(decoupled decay)")
        leaves = [p for g in self.param_groups for p in g["params"]]
        for p in leaves:
            if p.dtype in (torch.float16, torch.bfloat16):
                raise _lib.WaldoHipError(f"{name}: 16-bit parameters are not supported (no master weights), got {p.dtype}")
        if len({(p.device, p.dtype) for p in leaves}) != 1:
            raise ValueError(f"{name}: the parameters must share one device and dtype")
        self.device, dtype = leaves[0].device, leaves[0].dtype
        words = torch.float64 if dtype == torch.float64 else torch.float32
        self.scaler = scaler
        self.hyper = new_hyper(self.device, lr, betas, eps, max_norm, scaler, dtype=words)
        self.device_state = new_state(self.device, words)
        self._workspace = None
        self._plan = None

    # -- the step ------------------------------------------------------------------------------------------------------
    def _lists(self):
        out = [], [], [], [], []
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise ValueError(f"{type(self).__name__}: sparse gradients are not supported")
                st = self.state[p]
                if "exp_avg" not in st:
                    st["step"] = self.device_state[ST_STEP]  # (a view of the one counter)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                for lst, t in zip(out, (p, p.grad.contiguous(), st["exp_avg"], st["exp_avg_sq"], group["weight_decay"])):
                    lst.append(t)
        return out

    @torch.no_grad()
    def step(self, loss=None):
        """One step over the parameters that have a gradient; ``loss``: the step's loss, whose NaN skips it (the
        reference's test).  Reads nothing on the host."""
        if self._plan is not None and self._replan_needed():
            self._plan = None
        if self._plan is None:
            params, grads, ms, vs, wds = self._lists()
            if not params:
                return None
            if self.device.type != "cuda" or params[0].dtype != torch.float32:
                adam_step_(params, grads, ms, vs, self.device_state, self.hyper, weight_decays=wds, adamw=self._adamw,
                           loss=loss)
                return None
            # the first step over this set of parameters goes through the functional form and its checks; the host
            # arrays that do not change from step to step are kept (a step is host-bound on long lists otherwise)
            n = len(params)
            numels = (ctypes.c_int64 * n)(*[p.numel() for p in params])
            need = _lib.query("waldo_adam_workspace_bytes", n, numels)
            if self._workspace is None or self._workspace.numel() < need:
                self._workspace = torch.empty(max(need, 256), dtype=torch.uint8, device=self.device)
            adam_step_(params, grads, ms, vs, self.device_state, self.hyper, weight_decays=wds, adamw=self._adamw,
                       loss=loss, workspace=self._workspace)
            ptrs = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])  # noqa: E731
            everyone = [p for g in self.param_groups for p in g["params"]]
            self._plan = dict(params=params, others=[p for p in everyone if p.grad is None], n=n, numels=numels,
                              arrays=[ptrs(params), ptrs(grads), ptrs(ms), ptrs(vs)], decays=(ctypes.c_float * n)(*wds),
                              group_decays=[g["weight_decay"] for g in self.param_groups])
            return None
        plan = self._plan
        p_arr, g_arr = plan["arrays"][:2]
        keep = []
        for i, p in enumerate(plan["params"]):
            g = p.grad
            if not g.is_contiguous():
                g = g.contiguous()
                keep.append(g)
            p_arr[i], g_arr[i] = p.data_ptr(), g.data_ptr()
        if loss is not None:
            if loss.numel() != 1 or loss.device != self.device:
                raise ValueError(f"{type(self).__name__}.step: loss must be one element on {self.device}")
            loss = loss.detach()
            if loss.dtype != torch.float32:
                loss = loss.float()
        _launch(self.device, plan["arrays"], plan["numels"], plan["decays"], plan["n"], self.device_state, self.hyper,
                loss, self._workspace, self._adamw)
        return None

    def _replan_needed(self):
        """The set of parameters with a gradient differs from the kept plan's (or a gradient is sparse), or a group's
        weight decay has changed."""
        plan = self._plan
        return any(p.grad is None or p.grad.is_sparse for p in plan["params"]) or \
            any(p.grad is not None for p in plan["others"]) or \
            plan["group_decays"] != [g["weight_decay"] for g in self.param_groups]

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._plan = None

    def scale(self, loss):
        """``loss`` times the device's loss scale (``GradScaler.scale``)."""
        return loss * self.hyper[HY_SCALE].to(loss.dtype)

    def set_lr(self, lr):
        """A new learning rate (a float or a device tensor) for the next step, without a sync and without a recapture."""
        if torch.is_tensor(lr):
            self.hyper[HY_LR:HY_LR + 1].copy_(lr.detach().reshape(1), non_blocking=True)
        else:
            self.hyper[HY_LR:HY_LR + 1].fill_(float(lr))
            for g in self.param_groups:
                g["lr"] = float(lr)

    # -- device tensors: reading them is the caller's sync ---------------------------------------------------------------
    grad_norm = property(lambda self: self.device_state[ST_NORM], doc="the last step's gradient norm, unscaled")
    clip_coef = property(lambda self: self.device_state[ST_COEF])
    skipped = property(lambda self: self.device_state[ST_SKIPPED], doc="skipped steps in all")
    skipped_in_a_row = property(lambda self: self.device_state[ST_SKIP_ROW], doc="the reference's nancount")
    step_count = property(lambda self: self.device_state[ST_STEP], doc="finite steps so far")
    loss_scale = property(lambda self: self.hyper[HY_SCALE])

    # -- state in torch.optim.Adam's keys -------------------------------------------------------------------------------
    def state_dict(self):
        """``torch.optim.Adam``'s layout: per parameter ``step`` (a CPU scalar: this READS the device), ``exp_avg``,
        ``exp_avg_sq``.  The skip counters and the loss scale are not part of it."""
        sd = super().state_dict()
        step = self.device_state[ST_STEP].detach().to("cpu", torch.float32)
        sd["state"] = {k: dict(v, step=step.clone()) for k, v in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        """From this class or from ``torch.optim.Adam`` / ``AdamW``; every parameter's ``step`` must be the same number."""
        super().load_state_dict(state_dict)
        steps = {float(st["step"]) for st in self.state.values() if "step" in st}
        if len(steps) > 1:
            raise ValueError(f"{type(self).__name__}.load_state_dict: the parameters' step counts differ ({sorted(steps)}); "
                             "this optimizer keeps one count")
        self.device_state[ST_STEP] = steps.pop() if steps else 0.0
        self._plan = None
        for st in self.state.values():
            if "exp_avg" in st:
                st["step"] = self.device_state[ST_STEP]
                for k in ("exp_avg", "exp_avg_sq"):
                    st[k] = st[k].contiguous()
        # lr, betas and eps come with the groups; max_norm too when the dict is this class's (torch's has none: kept)
        g = self.param_groups[0]
        h = new_hyper("cpu", g["lr"], g["betas"], g["eps"], g.get("max_norm", 0), False, dtype=self.hyper.dtype)
        n = HY_SCALE if "max_norm" in g else HY_MAX_NORM
        self.hyper[:n].copy_(h[:n])

    def snapshot(self):
        """Clones of everything a step changes but the parameters (for ``restore``)."""
        return dict(state=self.device_state.clone(), hyper=self.hyper.clone(),
                    moments={p: (st["exp_avg"].clone(), st["exp_avg_sq"].clone()) for p, st in self.state.items()
                             if "exp_avg" in st})

    def restore(self, snap):
        """Back to ``snapshot()``'s values, in place; moments created since are zeroed."""
        self.device_state.copy_(snap["state"])
        self.hyper.copy_(snap["hyper"])
        for p, st in self.state.items():
            if "exp_avg" in st:
                m, v = snap["moments"].get(p, (None, None))
                st["exp_avg"].zero_() if m is None else st["exp_avg"].copy_(m)
                st["exp_avg_sq"].zero_() if v is None else st["exp_avg_sq"].copy_(v)


class AdamW(Adam):
    """``Adam`` with decoupled weight decay, ``p -= lr wd p`` before the update, per group (``torch.optim.AdamW``)."""

    _adamw = True


def add_weight_decay(net, weight_decay, skip_list=()):
    """The reference's decay / no-decay split (models/synthesizer.py:1091-1103): one-dimensional parameters, biases and
    the names of ``skip_list`` do not decay."""
    decay, no_decay = [], []
    for name, p in net.named_parameters():
        if not p.requires_grad:
            continue
        if p.ndim == 1 or name.endswith(".bias") or name.replace("module.", "") in skip_list:
            no_decay.append(p)
        else:
            decay.append(p)
    return [{"params": no_decay, "weight_decay": 0.0}, {"params": decay, "weight_decay": weight_decay}]


def from_opt(net, opt):
    """What the reference's ``create_optimizers`` builds for ``net`` (models/synthesizer.py:114-143) from ``optimizer``,
    ``lr``, ``beta1``, ``beta2``, ``wd``, ``clip_value`` and ``use_amp``: ``Adam`` (which, as there, ignores ``wd``) or
    ``AdamW`` with the no-decay split when the net has ``no_weight_decay()``.  None for no net or one without parameters
    (the reference's ``DummyOpt``)."""
    if net is None or not list(net.parameters()):
        return None
    kind = getattr(opt, "optimizer", "adam")
    common = dict(lr=opt.lr, betas=(opt.beta1, opt.beta2), max_norm=getattr(opt, "clip_value", 0),
                  scaler=bool(getattr(opt, "use_amp", False)))
    if kind == "adam":
        return Adam(net.parameters(), **common)
    if kind != "adamw":
        raise ValueError(f"from_opt: optimizer must be 'adam' or 'adamw', got {kind!r}")
    wd = getattr(opt, "wd", 0.0)
    inner = getattr(net, "module", net)
    if hasattr(inner, "no_weight_decay"):
        groups = [g for g in add_weight_decay(net, wd, inner.no_weight_decay()) if g["params"]]
        return AdamW(groups, weight_decay=0.0, **common)
    return AdamW(net.parameters(), weight_decay=wd, **common)


def resolve(optimizer, params, who):
    """The drivers' ``optimizer=`` argument: None, "adam", "adamw" or an ``Adam`` -> None or the optimizer."""
    if optimizer is None or isinstance(optimizer, Adam):
        return optimizer
    if optimizer == "adam":
        return Adam(params)
    if optimizer == "adamw":
        return AdamW(params)
    raise ValueError(f"{who}: optimizer must be None, 'adam', 'adamw' or an optim.Adam, got {optimizer!r}")
