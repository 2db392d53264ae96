"""Do the GPU cases of the token attention discriminate?  On the CPU: tests/token_attention_tiled.py restates what the
kernels compute, tile by tile, and takes one named fault at a time.  The restatement goes through the ``check`` helpers
of test_gpu_token_attention.py (forward) and test_gpu_token_attention_bwd.py (backward) -- the same operand lists, the
same ``close`` calls against ``token_attention_framework`` in fp32 and fp64 -- in place of the kernel.  Unfaulted it must
pass every case of every family; each fault must be rejected on at least one case of the family meant to catch it:

    fault               family that catches it                   side       what gives it away
    no_rescale          large scores                             forward    out keeps the weight of superseded maxima
    tail_unmasked       tile-edge grid, D = 16                   forward    exp(0 - m) per dead key in the row sum
    seam_off_by_one     tile-edge grid, D = 16                   forward    Nk2 = KT + 1: every key of segment two
    scale_ignored       scale family (EVERY case)                both       the precondition: out moves by > 100 TOL
    lse_without_log     tile-edge grid, D = 16                   backward   P too large by the row sum l
    query_tail_live     large scores, two rows far below zero    backward   exp(0 - lse) = inf times a zero operand
    dk_unscaled         tile-edge grid, D = 16; scale family     backward   grad k off by 1 / scale
    delta_other_order   one-key family                           backward   a rounding residue where dS is exactly 0

(tile sizes: 64 and 64, the kernels' -- a run without a GPU cannot query the limits; the GPU tests take them from the
library.)  Each rejection test prints how many cases rejected the fault and the worst distance / bound it reached."""
import pytest
import torch

import test_gpu_token_attention as FWD
import test_gpu_token_attention_bwd as BWD
from parity import TOL, _scale
from token_attention_tiled import FAULTS, attention

QT = KT = 64
CPU = "cpu"


def _family(name):
    """[(ops, scale, seed)] of a family, from the lists of the GPU files."""
    if name == "tile":
        return [(FWD.operands(CPU, *c[:6], seed=c[6]), None, c[6]) for c in FWD.tile_edge_cases(QT, KT, 16)]
    if name == "large":
        return [(FWD.large_score_operands(CPU, KT, low), None, 0) for low in FWD.LARGE_SCORE_CASES]
    if name == "scale":
        return [(FWD.operands(CPU, *c[:6], seed=c[6]), s, 0) for c, s in FWD.scale_cases(QT, KT)]
    assert name == "one"
    return [(FWD.operands(CPU, *c[:6], seed=c[6]), s, c[6]) for c, s in BWD.one_key_cases(QT)]


@pytest.fixture(scope="module")
def families():
    return {name: _family(name) for name in ("tile", "large", "scale", "one")}


def _judge(side, case, fn):
    ops, scale, seed = case
    if side == "forward":
        FWD.check(ops, "restatement", scale=scale, fn=fn)
    elif side == "backward":
        BWD.check(ops, "restatement", scale=scale, seed=seed, fn=fn)
    else:
        BWD.check_one_key(ops, scale, fn, seed)


@pytest.fixture
def ratios(monkeypatch):
    """Every distance / bound that ``close`` sees, as the checks of the two GPU files call it."""
    seen = []

    def recording(real):
        def close(a, b, tol=TOL, rel=False, what="", exact=None, **kw):
            a64, b64, e64 = (t.detach().double() for t in (a, b, exact))
            bound = tol * _scale(b64, rel, None) + (4.0 if rel else 2.0) * (b64 - e64).abs()
            r = torch.maximum((a64 - b64).abs(), (a64 - e64).abs()) / bound
            seen.append(float("inf") if not torch.isfinite(r).all() else r.max().item())
            return real(a, b, tol=tol, rel=rel, what=what, exact=exact, **kw)
        return close

    monkeypatch.setattr(FWD, "close", recording(FWD.close))
    monkeypatch.setattr(BWD, "close", recording(BWD.close))
    return seen


@pytest.mark.parametrize("side", ["forward", "backward"])
@pytest.mark.parametrize("name", ["tile", "large", "scale", "one"])
def test_the_restatement_passes_every_case(families, ratios, name, side):
    for case in families[name]:
        _judge(side, case, attention(None, QT, KT))
    print(f"[sensitivity] no fault, {name} {side}: worst {max(ratios):.3g} x its bound")
    assert max(ratios) <= 1.0


def test_the_restatement_passes_the_one_key_assertions(families):
    for case in families["one"]:
        _judge("one key", case, attention(None, QT, KT))


CATCHES = [("no_rescale", "large", "forward"), ("tail_unmasked", "tile", "forward"), ("seam_off_by_one", "tile", "forward"),
           ("scale_ignored", "scale", "forward"), ("scale_ignored", "scale", "backward"),
           ("lse_without_log", "tile", "backward"), ("query_tail_live", "large", "backward"),
           ("dk_unscaled", "tile", "backward"), ("dk_unscaled", "scale", "backward"),
           ("delta_other_order", "one", "one key")]


def test_every_fault_has_a_family():
    assert {c[0] for c in CATCHES} == set(FAULTS)


@pytest.mark.parametrize("fault,name,side", CATCHES)
def test_the_family_rejects_the_fault(families, ratios, fault, name, side):
    rejected = 0
    for case in families[name]:
        try:
            _judge(side, case, attention(fault, QT, KT))
        except AssertionError:
            rejected += 1
    worst = max(ratios, default=0.0)
    # (rejected with every ratio below 1: by an assertion ahead of ``close`` -- a non-finite gradient, a non-zero
    # element where 0 is exact)
    print(f"[sensitivity] {fault}, {name} {side}: rejected on {rejected} of {len(families[name])} cases, "
          + (f"worst {worst:.3g} x its bound" if worst > 1.0 else "by an assertion ahead of close"))
    assert rejected >= 1
    if fault == "scale_ignored":   # every case of the family moves the output by more than 100 TOL
        assert rejected == len(families[name])
