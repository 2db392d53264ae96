"""One training step of the future layer predictor as the reference runs it (``Synthesizer.generate_pose``,
models/synthesizer.py:681-779, at scripts/cityscapes/train_flp.sh: 4 clips of 14 frames of 128 x 256 per GPU, 4 context
frames, 16 objects + background, layout + flow input):

    under torch.no_grad():   encode_input(cat(lyt, flow)) -> estimate_layer(first ctx_len frames) -> estimate_pose
                             (the 7-tuple with last_obj, last_bg)                              (synthesizer.py:699-713)
    with autograd:           FLP(real poses, x_obj, x_bg, last_obj, last_bg, ctx_mask)         (synthesizer.py:716)
                             the three L1 terms on the frames to predict                       (synthesizer.py:752-754)
                             loss = 1 rec_obj_pose + 1 rec_bg_pose + 0.01 rec_occ_score, backward  (:755-762, 777)

The recipe pins ``min_ctx_length_vid`` = ``max_ctx_length_vid`` = 4, so the mask is "the first 4 frames of every clip":
``FLP.plan`` builds it from integers and ``supervision.pose_terms`` takes the plan, so nothing between the clip and the
parameter gradients reads the host, and ``graph=True`` replays the whole step from ONE HIP graph.  The clip is seeded
and resident on the device.  ``optimizer=None`` stops at the gradients: the optimizer, gradient clipping (``clip_value``
is 0 in the recipe) and the GradScaler are then the caller's.  ``optimizer="adam"`` / ``"adamw"`` / an ``optim.Adam`` ends
the step as the reference does (synthesizer.py:765-778) with ``optimizer.step(loss)`` -- the NaN test, the clip and the
update on the device (``waldo_amd.optim``), inside the graph when there is one.
"""
import torch

from .. import optim, supervision
from ..nets import FLP, LVD
from ..nets.flp import FlpPlan
from . import demo
from .lvd_step import recipe_net_opt
from .pipeline import synthetic_clip

OBJECTIVES = ("kernel", "framework")
# tools/options.py:446-448 and the LAST --s_lambda_rec_occ_score of train_flp.sh (:36; :15 says 0.1, argparse keeps the last)
RECIPE_WEIGHTS = {"rec_obj_pose": 1.0, "rec_bg_pose": 1.0, "rec_occ_score": 0.01}


def lvd_recipe_opt(**over):
    """``lvd_step.recipe_net_opt`` with what train_flp.sh changes against train_lvd.sh for the networks: the estimator's
    init mode (:24), and ``use_last_pose_decoder`` (:38), which makes ``estimate_pose`` hand out ``last_obj`` / ``last_bg``.
    (``oe_num_timesteps 5`` (:15) is train_lvd.sh's too; the clip's 14 frames are no option of the networks.)"""
    return recipe_net_opt(**dict(dict(pe_estimator_init_mode="zero", oe_num_timesteps=5, use_last_pose_decoder=True), **over))


def flp_recipe_opt(nopt=None, **over):
    """``nets.flp_net_opt`` at train_flp.sh next to LVD networks built from ``nopt`` (default: ``lvd_recipe_opt()``): the
    shared fields from ``nopt`` (512 wide, 8 heads, 16 objects, the rasters, the pose heads' constants), ``pg`` depths
    2 / 4 / 4 (tools/options.py:294-296), ``pg_num_timesteps 14`` (:15), ``use_last_pose_decoder`` and
    ``bg_mul_pose_decoder 1.2`` (:38), ``unconstrained_pose_decoder`` (:36), ``zero_init_dec`` at the reference's default
    (True, tools/options.py:323)."""
    d = dict(pg_com_depth=2, pg_enc_depth=4, pg_dec_depth=4, pg_num_timesteps=14, vid_len=14, use_last_pose_decoder=True,
             unconstrained_pose_decoder=True, bg_mul_pose_decoder=1.2, zero_init_dec=True)
    d.update(over)
    return demo.flp_demo_opt(lvd_recipe_opt() if nopt is None else nopt, **d)


class FlpStep:
    """``clips`` clips of ``frames`` frames resident on ``device`` (``lyt`` (B, T, 20, H, W), ``flow`` (B, T, 2, H, W));
    ``__call__`` runs the producers, ``FLP``, the objective and its backward once and returns the loss: FLP's parameters'
    ``.grad`` hold the gradients, ``terms`` the three scalars.  ``objective``: ``supervision.pose_terms`` through its
    kernel or through framework ops.  ``lvd_over`` / ``flp_over``: option fields that differ from the recipe's (smaller
    networks).  ``graph``: the step is captured once, here, and ``__call__`` replays it -- ``lyt`` and ``flow`` are the
    graph's inputs (new data written into them is a new step), the returned loss, ``terms`` and the gradients its
    outputs, overwritten by every replay.  ``optimizer``: None, "adam", "adamw" (the reference's defaults) or an
    ``optim.Adam`` over FLP's parameters; the step then ends in ``optimizer.step(loss)`` (in the graph too: a replay
    trains), and ``step.optimizer`` is it.  ``act_dtype``: the ``act_dtype`` of both networks (torch.bfloat16 /
    torch.float16: under autocast with the 16-bit attention kernel; the poses stay fp32)."""

    num_lyt = 20

    def __init__(self, clips, device, seed=0, frames=14, ctx_len=4, objective="kernel", graph=False, lvd_over=None,
                 flp_over=None, dim=128, aspect_ratio=2, optimizer=None, act_dtype=None):
        if objective not in OBJECTIVES:
            raise ValueError(f"FlpStep: objective must be one of {OBJECTIVES}, got {objective!r}")
        if not 0 < ctx_len < frames:
            raise ValueError(f"FlpStep: 0 < ctx_len < {frames} frames, got {ctx_len}")
        device = torch.device(device)
        if graph and device.type != "cuda":
            raise ValueError(f"FlpStep: graph=True needs a cuda device, got {device}")
        self.objective, self.clips, self.frames, self.ctx_len, self.device = objective, clips, frames, ctx_len, device
        # (lvd_demo_opt holds the options to its raster rule: frame / scale_factor / patch_size = latent_shape)
        shared = dict(dim=dim, aspect_ratio=aspect_ratio, ctx_len=ctx_len)
        self.lvd_opt = demo.lvd_demo_opt(lvd_recipe_opt(**dict(shared, **(lvd_over or {}))))
        self.flp_opt = flp_recipe_opt(self.lvd_opt, **(flp_over or {}))
        if self.flp_opt.pg_num_timesteps < frames:
            raise ValueError(f"FlpStep: {frames} frames, pg_num_timesteps is {self.flp_opt.pg_num_timesteps}")
        clip = demo.demo_opt(dim=dim, aspect_ratio=aspect_ratio, num_lyt=self.num_lyt)
        _, self.lyt = synthetic_clip(clip, clips, frames, seed, device)
        g = torch.Generator(device=device).manual_seed(seed + 1)
        self.flow = 0.05 * torch.randn(clips, frames, 2, *self.lyt.shape[-2:], generator=g, device=device)
        # (the networks from a generator state of their own: the clip above does not depend on their sizes)
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(seed)
            self.lvd = LVD(self.lvd_opt).to(device).eval()
            self.flp = FLP(self.flp_opt).to(device)
        self.lvd.act_dtype = self.flp.act_dtype = act_dtype
        for p in self.lvd.parameters():
            p.requires_grad_(False)
        self.leaves = list(self.flp.parameters())
        self.optimizer = optim.resolve(optimizer, self.leaves, "FlpStep")
        self.plan = self.flp.plan(clips, frames, ctx_len, device)
        self.terms = None
        self.graph = self._loss = None
        if graph:
            self._capture()

    def producers(self):
        """The no-grad half (synthesizer.py:699-713): ``FLP``'s seven inputs."""
        with torch.no_grad():
            x = self.lvd(input=torch.cat([self.lyt, self.flow], dim=2), mode="encode_input")
            x_obj, x_bg, _ = self.lvd(x=x[:, :self.ctx_len], mode="estimate_layer")
            obj_pose, bg_pose, occ_score, _, _, last_obj, last_bg = self.lvd(x=x, x_obj=x_obj, x_bg=x_bg,
                                                                             mode="estimate_pose")
        return obj_pose, bg_pose, occ_score, x_obj, x_bg, last_obj, last_bg

    def objective_terms(self, real, pred, ctx_mask):
        return supervision.pose_terms(real, pred, ctx_mask, fused=self.objective == "kernel")

    def _terms(self, ctx_mask):
        if ctx_mask is None:
            plan = mask = self.plan
        else:  # per-clip context lengths: one host read, in the plan
            plan = FlpPlan.from_mask(ctx_mask, self.flp.num_obj + 1, self.flp.cat_z)
            mask = ctx_mask
        inputs = self.producers()
        pred = self.flp(*inputs, ctx_mask=plan)
        return self.objective_terms(inputs[:3], pred, mask)

    def _step(self, ctx_mask=None):
        terms = self._terms(ctx_mask)
        loss = sum(RECIPE_WEIGHTS[k] * v for k, v in terms.items())
        loss.backward()
        # (detached: a term that kept the autograd graph alive would keep its AccumulateGrad nodes on this stream)
        self.terms = {k: v.detach() for k, v in terms.items()}
        loss = loss.detach()
        if self.optimizer is not None:
            self.optimizer.step(loss)
        return loss

    def _capture(self):
        """Two warm-up steps on a side stream, then the whole step -- producers, FLP, objective, backward -- captured in
        one graph.  The gradients are allocated inside the capture: they are the graph's buffers.  With an optimizer the
        warm-up steps train, so the parameters and the optimizer's state are put back before the capture."""
        if self.optimizer is not None:
            kept = [p.detach().clone() for p in self.leaves], self.optimizer.snapshot()
        side = torch.cuda.Stream(self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            for _ in range(2):
                self._step()
        torch.cuda.current_stream(self.device).wait_stream(side)
        if self.optimizer is not None:
            with torch.no_grad():
                for p, p0 in zip(self.leaves, kept[0]):
                    p.copy_(p0)
            self.optimizer.restore(kept[1])
        torch.cuda.synchronize(self.device)
        for p in self.leaves:
            p.grad = None
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            self._loss = self._step()
        self.graph = graph

    def __call__(self, ctx_mask=None):
        if self.graph is not None:
            if ctx_mask is not None:
                raise ValueError("FlpStep: a ctx_mask tensor costs a host read and runs eagerly only (graph=False)")
            self.graph.replay()
            return self._loss
        for p in self.leaves:
            p.grad = None
        return self._step(ctx_mask)

    def evaluate(self, ctx_mask=None):
        """The three terms and ``loss`` under ``no_grad`` (the recipe's ``--vid_metric "loss"``); eager."""
        with torch.no_grad():
            terms = self._terms(ctx_mask)
        return dict(terms, loss=sum(RECIPE_WEIGHTS[k] * v for k, v in terms.items()))

    def grads_finite(self):
        return all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in self.leaves)
