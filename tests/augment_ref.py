"""Restatement of the clip augmentation (include/waldo_hip.h "Clip augmentation") in torch ops on the CPU, in whatever
dtype is asked for (fp32: the reference the kernel is compared with; fp64: the exact one that measures the fp32
reference's own noise), and of the default branch of the reference's ``get_augmentation_parameters``
(data/base_dataset.py:113-165) in plain Python on given uniforms."""
import torch

ORDERS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))  # 0 brightness, 1 saturation, 2 hue


def reference_parameters(u, *, h, w, aspect_ratio, true_ratio, max_zoom, lr_flip, tb_flip, colorjitter, train=True):
    """data/base_dataset.py:114-115, 143-165 with ``random.random()`` replaced by the eight given numbers (in the
    order the reference draws them: v_flip, h_flip, zoom, top, left, brightness, saturation, hue; it draws no
    contrast under --colorjitter_no_contrast).  -> (flip bits, [top, left, h_crop, w_crop], [b, s, hue] or None, zoom)."""
    u_lr, u_tb, u_zoom, u_top, u_left, u_b, u_s, u_h = (float(v) for v in u)
    v_flip = u_lr > 0.5 if train and lr_flip else False
    h_flip = u_tb > 0.5 if train and tb_flip else False
    min_zoom = max(1., aspect_ratio / true_ratio)
    max_zoom = max(max_zoom, min_zoom)
    zoom = min_zoom + u_zoom * (max_zoom - min_zoom) if train else min_zoom
    h_crop = int(h / zoom)
    w_crop = int(h_crop * aspect_ratio)
    assert h >= h_crop and w >= w_crop
    top_crop = int(u_top * (h - h_crop)) if train else 0
    left_crop = int(u_left * (w - w_crop)) if train else 0
    jitter = None
    if colorjitter is not None and train:
        brightness = (u_b * 2 - 1) * colorjitter
        saturation = (u_s * 2 - 1) * colorjitter
        hue = 0.5 * (u_h * 2 - 1) * colorjitter
        jitter = [max(0, 1 + brightness), max(0, 1 + saturation), hue]
    return int(v_flip) | int(h_flip) << 1, [top_crop, left_crop, h_crop, w_crop], jitter, zoom


def clamped_box(box, hd, wd):
    top, left, hc, wc = (int(v) for v in box)
    top, left = min(max(top, 0), hd - 1), min(max(left, 0), wd - 1)
    return top, left, min(max(hc, 1), hd - top), min(max(wc, 1), wd - left)


def axis_taps(n_out, n_src, dtype, flipped=False, offset=None):
    """Source indices and weight of every output index along an axis resized from n_src to n_out: the position
    (o + 0.5) n_src / n_out - 0.5 clamped to [0, n_src - 1], the next index clamped too.  ``offset``: the output indices
    themselves (the flow's first resize is evaluated at given clip positions)."""
    o = torch.arange(n_out, dtype=dtype) if offset is None else offset.to(dtype)
    if flipped:
        o = (n_out - 1) - o
    scale = torch.tensor(float(n_src), dtype=dtype) / torch.tensor(float(n_out), dtype=dtype)
    s = ((o + 0.5) * scale - 0.5).clamp(0, n_src - 1)
    i0 = s.floor().long()
    return i0, (i0 + 1).clamp_max(n_src - 1), s - i0.to(dtype)


def blend(plane, ty, tx):
    """Bilinear blend of ``plane`` (..., H, W) at the taps of the two axes -> (..., len(ty), len(tx))."""
    (y0, y1, fy), (x0, x1, fx) = ty, tx
    fy = fy[:, None]
    r0, r1 = plane[..., y0, :], plane[..., y1, :]
    return (((1 - fy) * (1 - fx)) * r0[..., x0] + ((1 - fy) * fx) * r0[..., x1]) + \
           ((fy * (1 - fx)) * r1[..., x0] + (fy * fx) * r1[..., x1])


def rgb_to_hsv(r, g, b):
    maxc, minc = torch.maximum(r, torch.maximum(g, b)), torch.minimum(r, torch.minimum(g, b))
    eq = maxc == minc
    cr = maxc - minc
    ones = torch.ones_like(maxc)
    s = cr / torch.where(eq, ones, maxc)
    d = torch.where(eq, ones, cr)
    rc, gc, bc = (maxc - r) / d, (maxc - g) / d, (maxc - b) / d
    h = torch.where(maxc == r, bc - gc, torch.where(maxc == g, 2.0 + rc - bc, 4.0 + gc - rc))
    return torch.fmod(h / 6.0 + 1.0, 1.0), s, maxc, eq


def hsv_to_rgb(h, s, v):
    h6 = h * 6.0
    i = torch.floor(h6)
    f = h6 - i
    i = i.long() % 6
    p, q, t = (v * (1 - s)).clamp(0, 1), (v * (1 - s * f)).clamp(0, 1), (v * (1 - s * (1 - f))).clamp(0, 1)
    table = torch.stack([torch.stack(x) for x in ((v, q, p, p, t, v), (t, v, v, q, p, p), (p, p, t, v, v, q))])
    return table.gather(1, i.expand(3, 1, *i.shape)).squeeze(1)


def jitter_frame(u, order, jitter):
    """u (3, H, W) in [0, 1]; the three operations in the order ``order`` names (0..5; anything else: none)."""
    if not 0 <= int(order) <= 5:
        return u
    jb, js, jh = (jitter[k].to(u.dtype) for k in range(3))
    for op in ORDERS[int(order)]:
        if op == 0:
            u = (u * jb).clamp(0, 1)
        elif op == 1:
            grey = (0.299 * u[0] + 0.587 * u[1]) + 0.114 * u[2]
            u = (js * u + (1 - js) * grey).clamp(0, 1)
        else:
            h, s, v, eq = rgb_to_hsv(u[0], u[1], u[2])
            h = h + jh
            h = h - torch.floor(h)
            u = torch.where(eq, u, hsv_to_rgb(h, s, v))
    return u


def augment_ref(data, num_lyt, params, flow=None, out_size=None, dtype=torch.float64):
    """``data`` (B, T, Hd, Wd, 4) uint8, ``params`` with box / flip / jitter / order / zoom, ``flow`` (B, T, 2, Hf, Wf)
    or None -> (out (B, T, 3 + Nl, Ho, Wo), flow_out or None) in ``dtype``."""
    data = data.cpu()
    b, t, hd, wd, _ = data.shape
    ho, wo = (hd, wd) if out_size is None else out_size
    out = torch.empty(b, t, 3 + num_lyt, ho, wo, dtype=dtype)
    flow_out = None if flow is None else torch.empty(b, t, 2, ho, wo, dtype=dtype)
    box, flip, jitter, order, zoom = (getattr(params, k).cpu() for k in ("box", "flip", "jitter", "order", "zoom"))
    for i in range(b):
        top, left, hc, wc = clamped_box(box[i], hd, wd)
        lr, tb = bool(int(flip[i]) & 1), bool(int(flip[i]) & 2)
        ty, tx = axis_taps(ho, hc, dtype, tb), axis_taps(wo, wc, dtype, lr)
        for j in range(t):
            crop = data[i, j, top:top + hc, left:left + wc]
            u = blend(crop[..., :3].permute(2, 0, 1).to(dtype) / 255.0, ty, tx)
            u = jitter_frame(u, order[i, j], jitter[i])
            out[i, j, :3] = (u - 0.5) / 0.5
            onehot = (crop[..., 3].long()[None] == torch.arange(num_lyt)[:, None, None]).to(dtype)
            out[i, j, 3:] = 5.0 * (2.0 * blend(onehot, ty, tx) - 1.0)
            if flow is not None:
                src = flow[i, j].cpu().to(dtype)
                hf, wf = src.shape[-2:]
                # the first resize, to the clip's grid; then the frames' crop and resize
                full = blend(src, axis_taps(hd, hf, dtype), axis_taps(wd, wf, dtype))
                v = blend(full[:, top:top + hc, left:left + wc], ty, tx) * zoom[i].to(dtype)
                if lr:
                    v[0] = -v[0]
                if tb:
                    v[1] = -v[1]
                flow_out[i, j] = v
    return out, flow_out
