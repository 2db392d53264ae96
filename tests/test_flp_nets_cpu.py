"""CPU: ``waldo_amd.nets.FLP`` (LatentCompressor, PoseEncoder, PoseDecoder over the blocks of modules/transform.py) against
what the reference's own networks computed (tests/golden/flp_nets_reference.npz), through the suite's yardstick
``parity.close(got, ref32, exact=ref64)``; the plans that stand for ``ctx_mask``; the block types still refused.  On the
CPU every attention is the framework route (``WF.token_attention_clips_framework``)."""
import json

import pytest
import torch

import flp_nets_ref as R
from parity import close


@pytest.mark.parametrize("prefix", R.CASES)
def test_fixture_cases_load_strictly_and_reproduce_the_reference(prefix):
    opt, keys, d = R.case(prefix)
    with torch.no_grad():
        got = R.run(R.build(prefix, fused=False), d)
    R.check(close, got, d, prefix)
    mask = d["ctx_mask"]
    for name in R.OUTPUTS:   # the context frames come back as they went in
        assert torch.equal(got[name][mask], d["in." + name][mask]), name
    if not mask.all():
        assert (got["obj_pose"] - d["in.obj_pose"]).abs().max() > 0.1


def test_the_masks_of_the_fixture_differ_per_clip():
    counts = [R.case(p)[2]["ctx_mask"].sum(1).tolist() for p in R.CASES]
    assert sum(len(set(c)) > 1 for c in counts) >= 2
    assert any(R.case(p)[2]["ctx_mask"].all() for p in R.CASES)
    dims = {(R.case(p)[0]["embed_dim"] // R.case(p)[0]["num_heads"]) for p in R.CASES}
    assert dims == {16, 64}


@pytest.mark.parametrize("prefix", ["a_", "nocatz_"])
def test_fp64_networks_reproduce_the_fp64_reference(prefix):
    _, _, d = R.case(prefix)
    with torch.no_grad():
        got = R.run(R.build(prefix, fused=False, dtype=torch.float64), d, dtype=torch.float64)
    for name in R.OUTPUTS:
        assert got[name].dtype == torch.float64
        assert (got[name] - d[name + "64"]).abs().max().item() < 1e-10, name


@pytest.mark.parametrize("name", R.NOISE)
def test_noise_variants_have_the_recorded_keys(name):
    from waldo_amd.nets import FLP, flp_net_opt
    f = R.data()
    opt = json.loads(str(f[f"noise.{name}.opt"]))
    net = FLP(flp_net_opt(**opt))
    assert [k for k, _ in net.named_parameters()] == [str(k) for k in f[f"noise.{name}.keys"]]
    assert list(net.state_dict()) == [str(k) for k in f[f"noise.{name}.state_keys"]]
    # ... and run: finite outputs of the right shapes, the context frames untouched
    _, _, d = R.case("a_")
    net.fused = False
    with torch.no_grad():
        got = R.run(net.eval(), d)
    for k in R.OUTPUTS:
        assert got[k].shape == d["in." + k].shape and torch.isfinite(got[k]).all()
        assert torch.equal(got[k][d["ctx_mask"]], d["in." + k][d["ctx_mask"]])


def test_injected_noise_moves_the_output_by_its_strength():
    from waldo_amd.modules.transform import CrossAttention, FullAttention
    torch.manual_seed(0)
    x = torch.randn(3, 4, 32)
    mask = torch.tensor([[True, False, True], [False, True, False]])
    for attn, args in ((FullAttention(32, 2, None, True, flp=True), (x,)), (CrossAttention(32, 2, None, True), (x, x))):
        attn.fused = False
        assert attn.noise_strength.shape == () and attn.noise_strength.detach().item() == 0.0
        base = attn(*args, ctx_mask=mask)
        assert torch.equal(base, attn(*args, ctx_mask=mask))
        with torch.no_grad():
            attn.noise_strength.fill_(0.5)
        assert not torch.equal(base, attn(*args, ctx_mask=mask))


def test_the_integer_built_plan_is_the_mask_built_plan():
    from waldo_amd.modules.transform import ClipPlan
    b, t, ctx_len, n = 4, 14, 4, 17
    mask = (torch.arange(t) < ctx_len).expand(b, t)
    ints, masked = ClipPlan.first_frames(b, t, ctx_len, n), ClipPlan.from_mask(mask, n)
    for a, m in ((ints, masked), (ints.padded(), masked.padded()), (ints.complement(), masked.complement())):
        for name in ("index", "rest", "offsets", "rest_offsets", "mask"):
            assert torch.equal(getattr(a, name), getattr(m, name)), name
        assert (a.frames, a.rest_frames, a.batch, a.steps, a.tokens) == (m.frames, m.rest_frames, m.batch, m.steps, m.tokens)
        # the bounds hold for every clip; the integers' are tight
        for p in (a, m):
            assert int((p.offsets[1:] - p.offsets[:-1]).max()) <= p.max_len
            assert int((p.rest_offsets[1:] - p.rest_offsets[:-1]).max()) <= p.rest_max_len
    assert (ints.max_len, ints.rest_max_len) == (ctx_len * n, (t - ctx_len) * n)
    assert ints.padded().steps == t + 1 and ints.padded().frames == b * (ctx_len + 1)
    assert ints.offsets.dtype == torch.int32 and ints.index.dtype == torch.int64


def test_a_plan_of_an_irregular_mask_lists_the_frames_in_order():
    from waldo_amd.modules.transform import ClipPlan
    mask = torch.tensor([[1, 1, 0, 1, 0], [1, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 1, 1, 1, 1]], dtype=torch.bool)
    plan = ClipPlan.from_mask(mask, 3)
    assert plan.index.tolist() == torch.nonzero(mask.reshape(-1))[:, 0].tolist()
    assert plan.rest.tolist() == torch.nonzero(~mask.reshape(-1))[:, 0].tolist()
    assert plan.offsets.tolist() == [0, 9, 12, 12, 24] and plan.rest_offsets.tolist() == [0, 6, 18, 33, 36]
    pad = plan.padded()
    assert pad.mask[:, 0].all() and torch.equal(pad.mask[:, 1:], mask) and pad.frames == plan.frames + 4
    with pytest.raises(ValueError, match="boolean"):
        ClipPlan.from_mask(mask.float(), 3)
    with pytest.raises(ValueError, match="tokens"):
        ClipPlan.of(plan, 4)


def test_a_plan_in_place_of_the_mask_gives_the_same_outputs():
    from waldo_amd.nets import FlpPlan
    _, _, d = R.case("b_")
    net = R.build("b_", fused=False)
    opt = R.case("b_")[0]
    with torch.no_grad():
        want = R.run(net, d)
        got = R.run(net, d, ctx_mask=FlpPlan.from_mask(d["ctx_mask"], opt["num_obj"] + 1, opt["cat_z"]))
    for k in R.OUTPUTS:
        assert torch.equal(got[k], want[k])
    with pytest.raises(ValueError, match="cat_z"):
        R.run(net, d, ctx_mask=FlpPlan.from_mask(d["ctx_mask"], opt["num_obj"] + 1, not opt["cat_z"]))
    # "the first ctx_len frames" from integers is that mask's forward
    b, t = d["ctx_mask"].shape
    first = (torch.arange(t) < 2).expand(b, t)
    with torch.no_grad():
        want = R.run(net, d, ctx_mask=first)
        got = R.run(net, d, ctx_mask=net.plan(b, t, 2))
    for k in R.OUTPUTS:
        assert torch.equal(got[k], want[k])


def test_block_types_served_and_still_refused():
    from waldo_amd.modules.transform import Block, ClsAttention, CrossAttention, CustomAttention
    plain = dict(depth=1, dim=32, num_heads=2, norm_layer="ln", spectral_norm_layer=None, noise=False, dropout=0)
    args = dict(plain, flp=True)
    assert isinstance(CustomAttention("cross", **args).attn, CrossAttention)
    assert isinstance(CustomAttention("cls", **args).attn, ClsAttention)
    assert sorted(k for k, _ in CustomAttention("cross", **args).named_parameters()) == [
        "attn.kv.weight", "attn.proj.bias", "attn.proj.weight", "attn.q.weight"]
    assert "attn.attn.noise_strength" in dict(Block(block_type="full", **{**args, "noise": True}).named_parameters())
    # without the keyword the modules are the LVD networks': the predictor's block types, noise and ctx_mask are refused
    for block_type in ("cross", "cls"):
        with pytest.raises(NotImplementedError, match="flp=True"):
            Block(block_type=block_type, **plain)
    with pytest.raises(NotImplementedError, match="flp=True"):
        Block(block_type="full", **{**plain, "noise": True})
    with pytest.raises(NotImplementedError, match="ctx_mask"):
        Block(block_type="full", **plain)(torch.zeros(1, 4, 32), ctx_mask=torch.ones(1, 1, dtype=torch.bool))
    assert Block(block_type="full", **args)(torch.zeros(1, 4, 32), ctx_mask=torch.ones(1, 1, dtype=torch.bool)).shape == \
        (1, 4, 32)
    for block_type in ("ctx", "block_causal", "skip", "skip2"):
        with pytest.raises(NotImplementedError, match=block_type):
            Block(block_type=block_type, **args)
    with pytest.raises(ValueError, match="unknown block_type"):
        Block(block_type="nonsense", **args)
    with pytest.raises(NotImplementedError, match="spectral"):
        Block(block_type="cross", **{**args, "spectral_norm_layer": "sn"})
    with pytest.raises(ValueError, match="ctx_mask is required"):
        CrossAttention(32, 2, None, False)(torch.zeros(1, 4, 32), torch.zeros(1, 4, 32))
    with pytest.raises(ValueError, match="packed frames"):
        CrossAttention(32, 2, None, False)(torch.zeros(2, 4, 32), torch.zeros(1, 4, 32),
                                           ctx_mask=torch.tensor([[True, False]]))


def test_cls_attention_is_the_reference_sequence():
    """kv(cat[z_cls, x_ctx]) -> softmax over all N + 1 keys, spelled out."""
    from waldo_amd.modules.transform import ClsAttention
    torch.manual_seed(1)
    m = ClsAttention(32, 2, None)
    m.fused = False
    z, x = torch.randn(3, 1, 32), torch.randn(3, 5, 32)
    kv = m.kv(torch.cat([z, x], 1)).reshape(3, 6, 2, 2, 16).permute(2, 0, 3, 1, 4)
    q = m.q(z).reshape(3, 1, 2, 16).permute(0, 2, 1, 3)
    want = m.proj(((q @ kv[0].transpose(-2, -1) * m.scale).softmax(-1) @ kv[1]).transpose(1, 2).reshape(3, 1, 32))
    assert (m(z, x_ctx=x) - want).abs().max().item() < 1e-5


def test_flp_options():
    from waldo_amd.nets import FLP, flp_net_opt
    with pytest.raises(TypeError, match="unknown fields"):
        flp_net_opt(no_such_field=1)
    net = R.build("a_", fused=False)
    assert net.fused is False and not net.decode.self_blocks[0].fused and not net.compress.blocks.fused
    net.fused = True
    assert net.fused and net.encode.blocks.fused and net.decode.cross_blocks[0].fused
    _, _, d = R.case("a_")
    with pytest.raises(ValueError, match="ctx_mask is required"):
        net(*R.inputs(d))
    with pytest.raises(ValueError, match="mode"):
        net(*R.inputs(d), ctx_mask=d["ctx_mask"], mode="inference")
