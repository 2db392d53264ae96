"""LPIPS restated in plain functional ops from a state dict: the level chain (``normalize_tensor``, squared difference,
lin convolution, ``spatial_average``) and the two backbones, layer by layer in torchvision's ``features`` order.
Dtype-agnostic (the fp64 oracle of the GPU tests); written from the published structure of the ``lpips`` package, not
from ``waldo_amd/nets/lpips.py``.  A helper, not a test."""
import torch
import torch.nn.functional as F

EPS = 1e-10
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)

# torchvision's features, in order: ("conv", index, stride, pad), ("relu",), ("pool", kernel, stride), ("tap",)
VGG = [("conv", 0, 1, 1), ("relu",), ("conv", 2, 1, 1), ("relu",), ("tap",),
       ("pool", 2, 2), ("conv", 5, 1, 1), ("relu",), ("conv", 7, 1, 1), ("relu",), ("tap",),
       ("pool", 2, 2), ("conv", 10, 1, 1), ("relu",), ("conv", 12, 1, 1), ("relu",), ("conv", 14, 1, 1), ("relu",), ("tap",),
       ("pool", 2, 2), ("conv", 17, 1, 1), ("relu",), ("conv", 19, 1, 1), ("relu",), ("conv", 21, 1, 1), ("relu",), ("tap",),
       ("pool", 2, 2), ("conv", 24, 1, 1), ("relu",), ("conv", 26, 1, 1), ("relu",), ("conv", 28, 1, 1), ("relu",), ("tap",)]
ALEX = [("conv", 0, 4, 2), ("relu",), ("tap",),
        ("pool", 3, 2), ("conv", 3, 1, 2), ("relu",), ("tap",),
        ("pool", 3, 2), ("conv", 6, 1, 1), ("relu",), ("tap",),
        ("conv", 8, 1, 1), ("relu",), ("tap",),
        ("conv", 10, 1, 1), ("relu",), ("tap",)]
LAYERS = {"vgg": VGG, "alex": ALEX}
# the table of the issue: convolution index -> (slice, out, in, kernel)
CONVS = {
    "vgg": {0: (1, 64, 3, 3), 2: (1, 64, 64, 3), 5: (2, 128, 64, 3), 7: (2, 128, 128, 3), 10: (3, 256, 128, 3),
            12: (3, 256, 256, 3), 14: (3, 256, 256, 3), 17: (4, 512, 256, 3), 19: (4, 512, 512, 3), 21: (4, 512, 512, 3),
            24: (5, 512, 512, 3), 26: (5, 512, 512, 3), 28: (5, 512, 512, 3)},
    "alex": {0: (1, 64, 3, 11), 3: (2, 192, 64, 5), 6: (3, 384, 192, 3), 8: (4, 256, 384, 3), 10: (5, 256, 256, 3)},
}
WIDTHS = {"vgg": (64, 128, 256, 512, 512), "alex": (64, 192, 384, 256, 256)}


def expected_shapes(net):
    """The state dict of ``lpips.LPIPS(net=net)`` without the ``lins.*`` aliases: name -> shape."""
    shapes = {"scaling_layer.shift": (1, 3, 1, 1), "scaling_layer.scale": (1, 3, 1, 1)}
    for idx, (s, cout, cin, k) in CONVS[net].items():
        shapes[f"net.slice{s}.{idx}.weight"] = (cout, cin, k, k)
        shapes[f"net.slice{s}.{idx}.bias"] = (cout,)
    for k, c in enumerate(WIDTHS[net]):
        shapes[f"lin{k}.model.1.weight"] = (1, c, 1, 1)
    return shapes


def level(f0, f1, w, eps=EPS):
    """(N,): the chain at one level, ``w`` of C elements in any shape."""
    n0 = torch.sqrt((f0 * f0).sum(1, keepdim=True))
    n1 = torch.sqrt((f1 * f1).sum(1, keepdim=True))
    diff = (f0 / (n0 + eps) - f1 / (n1 + eps)) ** 2
    return (diff * w.reshape(1, -1, 1, 1)).sum(1).mean((1, 2))


def taps(net, state, x):
    slice_of = {idx: s for idx, (s, *_) in CONVS[net].items()}
    out = []
    for layer in LAYERS[net]:
        if layer[0] == "conv":
            _, idx, stride, pad = layer
            name = f"net.slice{slice_of[idx]}.{idx}"
            x = F.conv2d(x, state[name + ".weight"].to(x.dtype), state[name + ".bias"].to(x.dtype), stride=stride,
                         padding=pad)
        elif layer[0] == "relu":
            x = F.relu(x)
        elif layer[0] == "pool":
            x = F.max_pool2d(x, layer[1], layer[2])
        else:
            out.append(x)
    return out


def lpips(net, state, in0, in1, normalize=False):
    """(N, 1, 1, 1) from a state dict of ``expected_shapes(net)``; computed in the dtype of ``in0``."""
    if normalize:
        in0, in1 = 2 * in0 - 1, 2 * in1 - 1
    shift = torch.tensor(SHIFT, dtype=in0.dtype, device=in0.device).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=in0.dtype, device=in0.device).view(1, 3, 1, 1)
    t0 = taps(net, state, (in0 - shift) / scale)
    t1 = taps(net, state, (in1 - shift) / scale)
    total = 0
    for k in range(5):
        total = total + level(t0[k], t1[k], state[f"lin{k}.model.1.weight"].to(in0.dtype))
    return total.view(-1, 1, 1, 1)


def features(shape, seed, near=None, dtype=torch.float32):
    """A pair of |randn| feature maps; ``near``: f1 = f0 (1 + near randn)."""
    g = torch.Generator().manual_seed(seed)
    f0 = torch.randn(*shape, generator=g).abs()
    if near is None:
        f1 = torch.randn(*shape, generator=g).abs()
    else:
        f1 = f0 * (1 + near * torch.randn(*shape, generator=g))
    w = torch.rand(shape[1], generator=g) * (2.0 / shape[1])
    return f0.to(dtype), f1.to(dtype), w.to(dtype)
