"""Does the bound of the 16-bit token attention's backward (tests/token_attention_16bit_bwd.py) hold for the kernels'
arithmetic contract, and does it discriminate?  On the CPU: ``attention16_bwd`` restates the two matrix kernels tile by
tile in torch.  Unfaulted it must pass the bound on every case of the families test_gpu_token_attention_16bit_bwd.py runs
(tile edges at D = 16 / 32 / 64, scales, large scores) in both 16-bit types; with one planted fault at a time the bound
must REFUSE it on at least one case of the family meant for it:

    fault                                    family   what gives it away
    dk_ignores_the_scale                     scale    dK is off by 1 / scale wherever the scale is not 1
    delta_left_out                           tile     dS = P dP: dQ and dK of every case with more than one key
    lse_without_the_log                      tile     P is exp(log(l) - l) times too small
    seam_key_written_to_the_first_segment    tile     Nk2 present: row 0 of dK / dV and of dK2 / dV2
    second_segment_dropped                   tile     Nk2 present: dK2 / dV2 are zeros
    last_query_of_a_full_tile_dropped        tile     Nq >= 64: that query's share of every dK / dV
    live_rows_past_nq                        tile     Nq no multiple of 64: NaN in every dK / dV
    dq_scaled_twice                          scale    dQ is off by the scale

``delta_from_the_unrounded_out`` is shown NOT to be refused (the bound's E term is that difference).  The framework's
own 16-bit chain is refused.  The route switch is tested on the CPU.  (Tile size 64, the kernels'.)"""
import pytest
import torch

from token_attention_16bit_bwd import (DTYPES, FAMILIES, FAULTS, INDISTINGUISHABLE, KT, QT, attention16_bwd, bound_ratios,
                                       exact_and_bounds, family, framework_chain, within_bound)

CPU = "cpu"
MEANT_FOR = {"dk_ignores_the_scale": "scale", "dq_scaled_twice": "scale"}   # every other fault: "tile"
FAULT_DIMS = (32,)   # the faults are planted at one head dimension: the restatement has no path that depends on D


def fw(*a, **kw):
    from waldo_amd import functional
    return functional.token_attention_framework(*a, **kw)


@pytest.fixture(scope="module")
def cases():
    """(ops, grad_out, scale, what, (exact, bound)) per family and type: the fp64 references once for all the tests."""
    out = {}
    for dtype in DTYPES:
        for name in FAMILIES:
            out[name, dtype] = [(ops, go, s, what, exact_and_bounds(ops, go, s)) for ops, go, s, what in family(name, CPU, dtype)]
    return out


def worst(fn, case):
    ops, go, s, _, ref = case
    return max(bound_ratios(fn(*ops, grad_out=go, scale=s), *ref).values())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", FAMILIES)
def test_the_contract_passes_the_bound_on_every_case(cases, name, dtype):
    fn = attention16_bwd(None, QT, KT)
    per = {}
    for ops, go, s, what, ref in cases[name, dtype]:
        for k, r in bound_ratios(fn(*ops, grad_out=go, scale=s), *ref).items():
            per[k[:2]] = max(per.get(k[:2], 0.0), r)
    print(f"[bound16-bwd] the contract, {name} {dtype}: worst ratios {({k: round(r, 3) for k, r in per.items()})}")
    assert max(per.values()) <= 1.0, per


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_single_key_has_no_gradient_in_q_and_k(dtype):
    """P = 1: dS = dP - delta is the difference of two sums of the same products (O = V exactly), within the bound of 0."""
    ops, go, s, what = [c for c in family("tile", CPU, dtype, dims=(16,)) if c[0][1].shape[1] == 1 and c[0][3] is None][0]
    grads = attention16_bwd(None, QT, KT)(*ops, grad_out=go, scale=s)
    within_bound(grads, ops, go, s, what)
    assert grads[0].abs().max() < 1e-4 and grads[1].abs().max() < 1e-4


def test_the_framework_chain_in_16_bits_is_beyond_the_bound(cases):
    """So the framework route cannot pass for the kernel."""
    for dtype in DTYPES:
        refused = [c[3] for c in cases["large", dtype] + cases["scale", dtype] if worst(framework_chain(fw), c) > 1.0]
        print(f"[bound16-bwd] the framework's own chain {dtype}: refused on {len(refused)} cases")
        assert refused


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fault", FAULTS)
def test_the_bound_refuses_the_fault(cases, fault, dtype):
    fn = attention16_bwd(fault, QT, KT)
    name = MEANT_FOR.get(fault, "tile")
    meant = [c for c in cases[name, dtype] if c[0][0].shape[3] in FAULT_DIMS]
    refused = [(r, c[3]) for c in meant for r in [worst(fn, c)] if r > 1.0]
    print(f"[bound16-bwd] {fault} {dtype}: refused on {len(refused)} of {len(meant)} cases of the {name} family" +
          (f", first: {refused[0][1]} at {refused[0][0]:.3g} x its bound, worst {max(refused)[0]:.3g}" if refused else ""))
    assert refused, fault


@pytest.mark.parametrize("dtype", DTYPES)
def test_delta_from_the_unrounded_out_is_inside_the_bound(cases, dtype):
    """Documented, not claimed: the bound cannot tell the stored out from the unrounded one in delta."""
    fn = attention16_bwd(INDISTINGUISHABLE[0], QT, KT)
    meant = [c for c in cases["tile", dtype] if c[0][0].shape[3] in FAULT_DIMS] + cases["large", dtype]
    ratios = [worst(fn, c) for c in meant]
    print(f"[bound16-bwd] {INDISTINGUISHABLE[0]} {dtype}: worst {max(ratios):.3g} x the bound over {len(meant)} cases")
    assert max(ratios) <= 1.0


def test_the_route_switch_on_the_cpu():
    from waldo_amd import functional as WF
    assert WF.TOKEN_ATTENTION_16BIT_BACKWARD_ROUTES == ("framework", "kernel")
    assert WF.get_token_attention_16bit_backward_route() == "framework"
    with WF.token_attention_16bit_backward_route("kernel"):
        assert WF.get_token_attention_16bit_backward_route() == "kernel"
        with WF.token_attention_16bit_backward_route("framework"):                 # nests
            assert WF.get_token_attention_16bit_backward_route() == "framework"
        assert WF.get_token_attention_16bit_backward_route() == "kernel"
        assert WF.get_token_attention_16bit_route() == "framework"                  # the other switches stay put
        assert WF.get_token_attention_backward_route() == "framework"
    assert WF.get_token_attention_16bit_backward_route() == "framework"
    for bad in ("Kernel", "mfma", None, True, ""):
        with pytest.raises(ValueError, match="route must be one of"):
            WF.token_attention_16bit_backward_route(bad)
        assert WF.get_token_attention_16bit_backward_route() == "framework"
    with pytest.raises(RuntimeError, match="inside"):                               # restores on exception
        with WF.token_attention_16bit_backward_route("kernel"):
            raise RuntimeError("inside")
    assert WF.get_token_attention_16bit_backward_route() == "framework"
    try:                                                                            # a setter when not entered
        WF.token_attention_16bit_backward_route("kernel")
        assert WF.get_token_attention_16bit_backward_route() == "kernel"
    finally:
        WF.token_attention_16bit_backward_route("framework")
    assert WF.get_token_attention_16bit_backward_route() == "framework"


@pytest.mark.parametrize("dtype", DTYPES + (torch.float32,))
def test_cpu_tensors_are_unchanged_under_the_switch(dtype):
    from waldo_amd import functional as WF
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(2, 7, 3, 2, 16, generator=g).to(dtype)
    kv = torch.randn(2, 5, 2, 2, 16, generator=g).to(dtype)
    go = torch.randn(2, 7, 32, generator=g).to(dtype)

    def grads(fn):
        a, b = qkv.clone().requires_grad_(), kv.clone().requires_grad_()
        out = fn(*a.unbind(2), *b.unbind(2))
        out.backward(go)
        return out.detach(), a.grad, b.grad

    with WF.token_attention_16bit_route("kernel"), WF.token_attention_16bit_backward_route("kernel"):
        got = grads(WF.token_attention)
    for x, y in zip(got, grads(WF.token_attention_framework)):
        assert torch.equal(x, y)
