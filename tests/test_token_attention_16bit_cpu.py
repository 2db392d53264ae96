"""Does the bound of the 16-bit token attention (tests/token_attention_16bit.py) hold for the kernel's arithmetic contract,
and does it discriminate?  On the CPU: ``attention16`` restates the contract tile by tile in torch.  Unfaulted it must
pass the bound on every case of the tile-edge, scale and large-score families of test_gpu_token_attention.py, in both
16-bit types; with one planted fault at a time the bound must REFUSE it on at least one case:

    fault                              what gives it away
    last_key_of_a_full_tile_dropped    Nk1 = 64: the weight of key 63 is missing
    no_rescale                         large scores: out keeps the weight of superseded maxima
    seam_key_from_the_first_segment    Nk2 = 1, 65: the first key of segment two is another row
    scale_twice                        every case whose scale is not 1
    l_from_rounded_p                   the aligned-rounding recipe below (the three families do not catch it: the
                                       fault moves out by at most u |out|, inside u (A + |exact|) unless the
                                       roundings of p, of l and of the store all point one way)

(tile size 64, the kernels'; the GPU tests take it from the library.)"""
import math

import pytest
import torch

import test_gpu_token_attention as FWD
from token_attention_16bit import DTYPES, FAULTS, U, attention16, bound_ratio, exact_and_abs, to16, within_bound

QT = KT = 64
CPU = "cpu"


def fw(*a, **kw):
    from waldo_amd import functional
    return functional.token_attention_framework(*a, **kw)


def aligned_rounding_operands(dtype, d=64, nm=600, sigma=9.0):
    """Operands on which the roundings of p line up, with logits spread over sigma = 9 like a sharp softmax: component 0
    of q carries the scores, so key x's weight is p(x) = exp(scale q0 (x - xmax)).  Searched among the representable
    x: one value M whose p rounds DOWN by nearly a full u (``nm`` keys, values 0: they carry the row sum), one value P
    whose p rounds UP by nearly u (one key, values near 1: it carries out), and the maximum (one key, values 0).  The
    contract's out is then high by u from p's rounding; summing l from the rounded p lowers l by u on top of that, and
    the store's rounding of one of the D columns adds its own u."""
    u = U[dtype]
    q0, scale = 8.0, d ** -0.5
    xs = torch.arange(-4.0, 0.0, 2.0 ** -6).to(dtype).unique()              # representable in both types
    p = torch.exp((xs.float() * q0) * torch.tensor(scale) - 0.0)            # the maximum key has x = 0
    rel = (p.to(dtype).double() - p.double()) / p.double() / u
    keep = p > math.exp(-sigma)
    im, ip = int(torch.where(keep, rel, 9.0).argmin()), int(torch.where(keep, rel, -9.0).argmax())
    assert rel[im] < -0.8 and rel[ip] > 0.8, (rel[im], rel[ip])
    nk = nm + 2
    q = torch.zeros(1, 4, 1, d)
    q[..., 0] = q0
    k, v = torch.zeros(1, nk, 1, d), torch.zeros(1, nk, 1, d)
    k[0, 1, 0, 0] = xs[ip].float()                                          # key 0 is the maximum: m is final at once
    k[0, 2:, 0, 0] = xs[im].float()
    v[0, 1, 0] = 2.0 ** 12 * (1.0 + torch.arange(d) * 2.0 ** -7)            # representable (8 significant bits), and
    #                                                                         large: out and A are of order 10, so that
    #                                                                         u A stands far above the bound's TOL term
    return to16((q, k, v, None, None), dtype)


def _family(name, dtype):
    """[(ops, scale, what)] of a family, from the lists of the fp32 GPU file, rounded to ``dtype``."""
    if name == "tile":
        return [(to16(FWD.operands(CPU, *c[:6], seed=c[6]), dtype), None, f"tile {c}")
                for d in (16, 32, 64) for c in FWD.tile_edge_cases(QT, KT, d)]
    if name == "scale":
        return [(to16(FWD.operands(CPU, *c[:6], seed=c[6]), dtype), s, f"scale {c} {s:.3g}")
                for c, s in FWD.scale_cases(QT, KT)]
    if name == "large":
        return [(to16(FWD.large_score_operands(CPU, KT, low), dtype), None, f"large scores, low rows {low}")
                for low in FWD.LARGE_SCORE_CASES]
    assert name == "aligned"
    return [(aligned_rounding_operands(dtype), None, "aligned roundings")]


FAMILIES = ("tile", "scale", "large", "aligned")


@pytest.fixture(scope="module")
def cases():
    """(ops, scale, what, exact, A) per family and type: the fp64 references once for all the tests."""
    out = {}
    for dtype in DTYPES:
        for name in FAMILIES:
            out[name, dtype] = [(ops, s, what, *exact_and_abs(fw, *ops, scale=s)) for ops, s, what in _family(name, dtype)]
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", FAMILIES)
def test_the_contract_passes_the_bound_on_every_case(cases, name, dtype):
    fn = attention16(None, KT)
    worst = max(bound_ratio(fn(*ops, scale=s), exact, a)[0] for ops, s, _, exact, a in cases[name, dtype])
    print(f"[bound16] the contract, {name} {dtype}: worst {worst:.3g} x its bound")
    assert worst <= 1.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_single_key_gives_its_value_exactly(dtype):
    for nq in (1, 17, 65):
        ops = to16(FWD.operands(CPU, 2, 2, nq, 1, None, 32, seed=3), dtype)
        assert torch.equal(attention16(None, KT)(*ops), ops[2].reshape(2, 1, 64).expand(2, nq, 64))


def test_the_framework_chain_in_16_bits_is_beyond_the_bound():
    """So the framework route cannot pass for the kernel: it rounds the scores."""
    for dtype in DTYPES:
        ops = to16(FWD.large_score_operands(CPU, KT), dtype)
        with pytest.raises(AssertionError):
            within_bound(fw, fw(*ops), ops, what="the framework's own 16-bit chain")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fault", FAULTS)
def test_the_bound_refuses_the_fault(cases, fault, dtype):
    fn = attention16(fault, KT)
    refused = []
    for name in FAMILIES:
        for ops, s, what, exact, a in cases[name, dtype]:
            r = bound_ratio(fn(*ops, scale=s), exact, a)[0]
            if r > 1.0:
                refused.append((r, what))
    print(f"[bound16] {fault} {dtype}: refused on {len(refused)} cases" +
          (f", first: {refused[0][1]} at {refused[0][0]:.3g} x its bound, worst {max(refused)[0]:.3g}" if refused else ""))
    assert refused, fault
