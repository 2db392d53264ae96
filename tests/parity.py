"""The bound every GPU parity test of a CHAIN uses: the north star's 1e-4 plus a MEASURED allowance for
the fp32 reference's own rounding noise on the same input -- never a typed one.

``exact`` is the same quantity evaluated by the oracle in float64 from the same fp32 inputs (the
oracles are dtype-agnostic restatements).  |ref32_i - exact_i| measures how far the fp32 reference
itself is from exact arithmetic at ELEMENT i: two fp32 evaluations with different summation orders
or fused multiply-adds cannot agree better than that, so k times it is added to that element's budget
(k = 2 for outputs, 4 for gradients, whose integrands jump at texel boundaries):

    bound_i = tol * scale_i + k * |ref32_i - exact_i|

The noise is per element, not the tensor's maximum: one sample that lands within an ulp of a texel
boundary moves the few elements downstream of it, and must not widen the bound of every other one.
``scale_i`` is 1 for outputs; with ``rel`` it is the largest |ref32| of the tensor, or with
``slice_dims`` of the element's slice (a frame, a layer, an object), floored at 1e-2 of the tensor's,
so that a small layer is judged against its own magnitude.  (A comparison against a reference at its
own sample positions on a large raster may take the tensor's maximum noise instead: ``noise_of``.)  The HIP result must be within bound_i of
ref32 AND of exact.  ``exempt`` marks elements that the fp64 oracle finds downstream of a measured
kink (a branch of the chain decided within rounding of its threshold); only those may sit up to 25 x
over their bound.  Every comparison prints its distances, the largest bound / scale and its worst
element by index (pytest -s / on failure)."""
import torch

TOL = 1e-4
KINK_CAP = 25.0


def _scale(b, rel, slice_dims):
    if not rel:
        return torch.ones_like(b)
    full = max(b.abs().max().item(), 1e-30)
    if not slice_dims:
        return torch.full_like(b, full)
    red = [d for d in range(b.dim()) if d not in tuple(d % b.dim() for d in slice_dims)]
    s = b.abs().amax(dim=red, keepdim=True) if red else b.abs()
    return s.clamp_min(1e-2 * full).expand_as(b)


def close(a, b, tol=TOL, rel=False, what="", exact=None, slice_dims=None, exempt=None, noise_of="element"):
    """``noise_of="tensor"``: the noise term is the tensor's max |ref32 - exact| for every element, for comparisons
    against a reference evaluated at its OWN sample positions on large rasters (or with another summation order of
    thousands of terms), where the implementation's rounding of a position -- or of a long sum -- moves elements
    whose own fp32 noise happens to be small."""
    if a is None or b is None:
        assert a is None and b is None, what
        return
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.numel() == 0:
        return
    scale = _scale(b, rel, slice_dims)
    err = (a - b).abs()
    if exact is None:
        noise = torch.zeros_like(b)
        err64 = err
    else:
        e64 = exact.detach().cpu().double()
        assert e64.shape == b.shape, (what, e64.shape, b.shape)
        noise = (b - e64).abs()
        if noise_of == "tensor":
            noise = torch.full_like(noise, noise.max().item())
        else:
            assert noise_of == "element", noise_of
        err64 = (a - e64).abs()
    bound = tol * scale + (4.0 if rel else 2.0) * noise
    cap = bound
    if exempt is not None:
        exempt = torch.as_tensor(exempt, dtype=torch.bool).cpu().expand_as(b)
        cap = torch.where(exempt, KINK_CAP * bound, bound)
    ratio = torch.maximum(err, err64) / bound
    worst = int(ratio.argmax())
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(worst), b.shape))
    # an element passes only when both distances are PROVABLY within its cap: a NaN anywhere -- in the candidate,
    # the reference or the bound -- fails every comparison and so fails the element
    over = ~((err <= cap) & (err64 <= cap))
    n_ex = 0 if exempt is None else int(exempt.sum())
    print(f"[parity] {what}: |hip-ref32| {err.max().item():.3e}  |hip-ref64| {err64.max().item():.3e}  "
          f"|ref32-ref64| {noise.max().item():.3e}  bound/scale {(bound / scale).max().item():.2e}  "
          f"worst {ratio.reshape(-1)[worst].item():.3g} x its bound at {idx}"
          + (f"  ({n_ex} kink-exempt elements)" if n_ex else ""))
    if over.any():
        i = int((torch.maximum(err, err64) / cap).argmax())
        at = tuple(int(j) for j in torch.unravel_index(torch.tensor(i), b.shape))
        raise AssertionError(
            f"{what}: {int(over.sum())} of {b.numel()} elements beyond their bound; the worst at {at}: "
            f"hip {a.reshape(-1)[i].item():.6e}  ref32 {b.reshape(-1)[i].item():.6e}"
            + ("" if exact is None else f"  ref64 {e64.reshape(-1)[i].item():.6e}")
            + f"  bound {cap.reshape(-1)[i].item():.3e} (tol*scale {(tol * scale).reshape(-1)[i].item():.1e}, "
              f"fp32 noise {noise.reshape(-1)[i].item():.1e})")


def compare_warp_composite(got, m32, m64):
    """The fused warp / composite's (rgb, alpha, grad_layers, grad_pts, grad_occ) -- entries may be None -- against
    the oracle sampled at the implementation's OWN coordinates (oracle/wif_oracle.py:warp_composite_px) in fp32
    (m32) and fp64 (m64): every floor and in-range decision is the implementation's, so what is left between them
    is arithmetic.  Each output per element with its measured fp32 noise (the two gradients per (frame, layer)
    slice); rgb, alpha and the control-point gradient -- discontinuous where a sample crosses a texel boundary,
    several per cent of its scale against a reference that rounds one sample to the other side -- also against
    m64 at plain TOL * scale."""
    names = ("rgb", "alpha", "grad_layers", "grad_pts", "grad_occ")
    for i, name in enumerate(names):
        if got[i] is None:
            continue
        close(got[i], m32[i], rel=i >= 2, what=name, exact=m64[i], slice_dims=(0, 1) if i in (2, 4) else None)
        if i in (0, 1, 3):
            close(got[i], m64[i], rel=i >= 2, what=name + " vs fp64 at the kernel's coordinates")
