"""Restatement of the face detector (csrc/detect.hip, vspbfr_amd/detect.py) for the tests: the RetinaFace / MobileNet-0.25
network as a plain torch.nn tree with the checkpoint's key names, evaluated in float64 or float32 on the CPU, and priors, decode,
candidate selection and greedy NMS in NumPy at either precision.  Nothing here imports the product."""
import numpy as np
import torch
import torch.nn as nn

MEAN_BGR = (104.0, 117.0, 123.0)
STEPS = (8, 16, 32)
MIN_SIZES = ((16, 32), (64, 128), (256, 512))
CAND_CAPPED, FACES_CAPPED, NONFINITE = 1, 2, 4


def cbl(i, o, s, a):
    return nn.Sequential(nn.Conv2d(i, o, 3, s, 1, bias=False), nn.BatchNorm2d(o), nn.LeakyReLU(a))


def cb(i, o):
    return nn.Sequential(nn.Conv2d(i, o, 3, 1, 1, bias=False), nn.BatchNorm2d(o))


def c1(i, o, a):
    return nn.Sequential(nn.Conv2d(i, o, 1, 1, 0, bias=False), nn.BatchNorm2d(o), nn.LeakyReLU(a))


def dw(i, o, s):
    return nn.Sequential(nn.Conv2d(i, i, 3, s, 1, groups=i, bias=False), nn.BatchNorm2d(i), nn.LeakyReLU(0.1),
                         nn.Conv2d(i, o, 1, bias=False), nn.BatchNorm2d(o), nn.LeakyReLU(0.1))


class Body(nn.Module):
    def __init__(self):
        super().__init__()
        self.stage1 = nn.Sequential(cbl(3, 8, 2, 0.1), dw(8, 16, 1), dw(16, 32, 2), dw(32, 32, 1), dw(32, 64, 2), dw(64, 64, 1))
        self.stage2 = nn.Sequential(dw(64, 128, 2), *[dw(128, 128, 1) for _ in range(5)])
        self.stage3 = nn.Sequential(dw(128, 256, 2), dw(256, 256, 1))

    def forward(self, x):
        a = self.stage1(x)
        b = self.stage2(a)
        return a, b, self.stage3(b)


def nearest(x, h, w):
    """nearest upsampling with source index floor(i in / out), as integers"""
    iy = (torch.arange(h) * x.shape[2]) // h
    ix = (torch.arange(w) * x.shape[3]) // w
    return x[:, :, iy][:, :, :, ix]


class FPN(nn.Module):
    def __init__(self):
        super().__init__()
        self.output1, self.output2, self.output3 = c1(64, 64, 0.1), c1(128, 64, 0.1), c1(256, 64, 0.1)
        self.merge1, self.merge2 = cbl(64, 64, 1, 0.1), cbl(64, 64, 1, 0.1)

    def forward(self, a, b, c):
        o3 = self.output3(c)
        o2 = self.output2(b)
        o2 = self.merge2(o2 + nearest(o3, o2.shape[2], o2.shape[3]))
        o1 = self.output1(a)
        o1 = self.merge1(o1 + nearest(o2, o1.shape[2], o1.shape[3]))
        return o1, o2, o3


class SSH(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv3X3 = cb(64, 32)
        self.conv5X5_1 = cbl(64, 16, 1, 0.1)
        self.conv5X5_2 = cb(16, 16)
        self.conv7X7_2 = cbl(16, 16, 1, 0.1)
        self.conv7x7_3 = cb(16, 16)

    def forward(self, x):
        t = self.conv5X5_1(x)
        return torch.relu(torch.cat([self.conv3X3(x), self.conv5X5_2(t), self.conv7x7_3(self.conv7X7_2(t))], dim=1))


class Head(nn.Module):
    def __init__(self, n):
        super().__init__()
        self.conv1x1 = nn.Conv2d(64, n, 1)

    def forward(self, x):
        y = self.conv1x1(x).permute(0, 2, 3, 1).contiguous()
        return y.view(y.shape[0], -1, y.shape[3] // 2)


class RetinaFace(nn.Module):
    def __init__(self):
        super().__init__()
        self.body, self.fpn = Body(), FPN()
        self.ssh1, self.ssh2, self.ssh3 = SSH(), SSH(), SSH()
        self.ClassHead = nn.ModuleList([Head(4) for _ in range(3)])
        self.BboxHead = nn.ModuleList([Head(8) for _ in range(3)])
        self.LandmarkHead = nn.ModuleList([Head(20) for _ in range(3)])

    def features(self, x):
        o = self.fpn(*self.body(x))
        return [ssh(f) for ssh, f in zip((self.ssh1, self.ssh2, self.ssh3), o)]

    def forward(self, x):
        f = self.features(x)
        return tuple(torch.cat([h(v) for h, v in zip(heads, f)], dim=1) for heads in (self.ClassHead, self.BboxHead, self.LandmarkHead))


def make_model(seed, class_bias=0.0):
    """A float64 RetinaFace in eval mode with well-conditioned random weights: convolutions N(0, 1 / fan_in) (the first one divided by
    64: its input is in grey levels), BatchNorm scale and variance in 0.75..1.25 with small shift and mean, head biases N(0, 0.3^2);
    class_bias is added to the background logit's bias (fewer candidates)."""
    g = torch.Generator().manual_seed(seed)
    net = RetinaFace().double().eval()
    first = True
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.Conv2d):
                fan_in = m.weight.shape[1] * m.weight.shape[2] * m.weight.shape[3]
                m.weight.copy_(torch.randn(m.weight.shape, generator=g, dtype=torch.float64) / fan_in ** 0.5 / (64.0 if first else 1.0))
                first = False
                if m.bias is not None:
                    m.bias.copy_(0.3 * torch.randn(m.bias.shape, generator=g, dtype=torch.float64))
            elif isinstance(m, nn.BatchNorm2d):
                n = m.weight.shape[0]
                m.weight.copy_(0.75 + 0.5 * torch.rand(n, generator=g, dtype=torch.float64))
                m.bias.copy_(0.1 * torch.randn(n, generator=g, dtype=torch.float64))
                m.running_mean.copy_(0.1 * torch.randn(n, generator=g, dtype=torch.float64))
                m.running_var.copy_(0.75 + 0.5 * torch.rand(n, generator=g, dtype=torch.float64))
        for h in net.ClassHead:
            h.conv1x1.bias[0::2] += class_bias
    return net


def as_f32(net):
    """a float32 copy of the model (the fp32 CPU evaluation of the error bound)"""
    import copy
    return copy.deepcopy(net).float()


def canvas(photos, Hc, Wc, dtype=torch.float64):
    """uint8 (h, w, 3) RGB photos -> (B, 3, Hc, Wc): BGR minus the mean at the top-left, zero elsewhere"""
    x = torch.zeros((len(photos), 3, Hc, Wc), dtype=dtype)
    mean = torch.tensor(MEAN_BGR, dtype=dtype).view(3, 1, 1)
    for k, a in enumerate(photos):
        a = np.asarray(a)
        t = torch.from_numpy(a[:, :, ::-1].copy()).permute(2, 0, 1).to(dtype)
        x[k, :, :a.shape[0], :a.shape[1]] = t - mean
    return x


def test_photo(h, w, seed):
    """a smooth random uint8 (h, w, 3) photo"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.zeros((h, w, 3))
    for c in range(3):
        for _ in range(4):
            fx, fy, ph = rng.uniform(0.01, 0.2), rng.uniform(0.01, 0.2), rng.uniform(0, 6.28)
            img[:, :, c] += rng.uniform(10, 40) * np.sin(fx * xx + fy * yy + ph)
    img += 128.0 + rng.normal(0.0, 6.0, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------------- post-processing
def level_sizes(Hc, Wc):
    return [(-(-Hc // s), -(-Wc // s)) for s in STEPS]


def priors(Hc, Wc, dtype=np.float64):
    """(cx, cy, m) of every prior, each (P,): level, then cell in raster order, then the two anchor sizes"""
    cx, cy, mm = [], [], []
    for (h, w), step, sizes in zip(level_sizes(Hc, Wc), STEPS, MIN_SIZES):
        i, j = np.mgrid[0:h, 0:w]
        for arr, v in ((cx, (j + 0.5) * step), (cy, (i + 0.5) * step)):
            arr.append(np.repeat(v.reshape(-1), 2))
        mm.append(np.tile(np.asarray(sizes, dtype=np.float64), h * w))
    return tuple(np.concatenate(a).astype(dtype) for a in (cx, cy, mm))


def decode(conf, loc, lm, Hc, Wc, dtype=np.float64):
    """one image: conf (P, 2), loc (P, 4), lm (P, 10) -> (score (P,), box (P, 4) x1 y1 x2 y2, pts (P, 10)) in canvas pixels, all
    arithmetic in `dtype`"""
    conf, loc, lm = (np.asarray(a).astype(dtype) for a in (conf, loc, lm))
    cx, cy, m = priors(Hc, Wc, dtype)
    one, tenth, fifth, half = dtype(1.0), dtype(0.1), dtype(0.2), dtype(0.5)
    with np.errstate(over="ignore", invalid="ignore"):
        score = one / (one + np.exp(conf[:, 0] - conf[:, 1]))
        v = tenth * m
        bx, by = cx + loc[:, 0] * v, cy + loc[:, 1] * v
        bw, bh = m * np.exp(fifth * loc[:, 2]), m * np.exp(fifth * loc[:, 3])
        box = np.stack([bx - half * bw, by - half * bh, bx + half * bw, by + half * bh], axis=1)
        c = np.stack([cx, cy] * 5, axis=1)
        pts = c + lm * v[:, None]
    return score.astype(dtype), box.astype(dtype), pts.astype(dtype)


def iou_matrix(box):
    """pairwise IoU with plain areas (no + 1), in the boxes' dtype"""
    x1, y1, x2, y2 = (box[:, k] for k in range(4))
    zero = box.dtype.type(0)
    iw = np.maximum(np.minimum(x2[:, None], x2[None]) - np.maximum(x1[:, None], x1[None]), zero)
    ih = np.maximum(np.minimum(y2[:, None], y2[None]) - np.maximum(y1[:, None], y1[None]), zero)
    inter = iw * ih
    area = (x2 - x1) * (y2 - y1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return inter / (area[:, None] + area[None] - inter)


def select_nms(score, box, pts, threshold, nms, max_candidates=1024, max_faces=256):
    """-> dict(keep: prior indices of the kept faces in order, status, candidates, nonfinite, order: the surviving candidates in order).
    Candidates: score > threshold with finite box and landmarks; the first max_candidates in (score descending, prior ascending);
    greedy NMS in that order, suppressed when IoU with a kept one > nms; at most max_faces are kept."""
    thr, nm = score.dtype.type(threshold), score.dtype.type(nms)
    above = score > thr
    finite = np.isfinite(box).all(axis=1) & np.isfinite(pts).all(axis=1)
    cand = np.flatnonzero(above & finite)
    nbad = int((above & ~finite).sum())
    order = cand[np.lexsort((cand, -score[cand].astype(np.float64)))]
    status = (CAND_CAPPED if len(order) > max_candidates else 0) | (NONFINITE if nbad else 0)
    order = order[:max_candidates]
    iou = iou_matrix(box[order])
    keep, removed = [], np.zeros(len(order), dtype=bool)
    for i in range(len(order)):
        if removed[i]:
            continue
        if len(keep) == max_faces:
            status |= FACES_CAPPED
            break
        keep.append(i)
        removed[i + 1:] |= iou[i, i + 1:] > nm
    return {"keep": order[keep].astype(np.int64), "status": status, "candidates": int(len(cand)), "nonfinite": nbad, "order": order}


def margins(score, box, threshold, nms, order):
    """(smallest |score - threshold| over all priors, smallest |IoU - nms| over the pairs of surviving candidates)"""
    s = float(np.nanmin(np.abs(score.astype(np.float64) - threshold)))
    if len(order) < 2:
        return s, float("inf")
    iou = iou_matrix(box[order].astype(np.float64))
    iu = np.triu_indices(len(order), 1)
    return s, float(np.nanmin(np.abs(iou[iu] - nms)))


def to_photo(xy, h, w, hr, wr):
    """canvas coordinates (..., 2) -> photo pixels under the pixel-centre convention: x (w / w') - 0.5"""
    return np.asarray(xy, dtype=np.float64) * np.array([w / wr, h / hr], dtype=np.float64) - 0.5


# ------------------------------------------------------------------------------------------------------------- single layers, any dtype
def lrelu(x, slope):
    return x if slope is None else torch.where(x < 0, x * slope, x)


def entry_ref(photos, Hc, Wc, w, b, dtype, slope=0.1):
    """w (8, 3, 3, 3), b (8): the first layer on the canvas of `photos`"""
    return lrelu(torch.nn.functional.conv2d(canvas(photos, Hc, Wc, dtype), w.to(dtype), b.to(dtype), stride=2, padding=1), slope)


def sep_ref(x, wd, bd, wp, bp, stride, dtype, slope=0.1):
    """wd (C, 1, 3, 3), bd (C), wp (Co, C, 1, 1), bp (Co)"""
    F = torch.nn.functional
    t = lrelu(F.conv2d(x.to(dtype), wd.to(dtype), bd.to(dtype), stride=stride, padding=1, groups=x.shape[1]), slope)
    return lrelu(F.conv2d(t, wp.to(dtype), bp.to(dtype)), slope)


def conv3x3_ref(x, w, b, slope, dtype):
    return lrelu(torch.nn.functional.conv2d(x.to(dtype), w.to(dtype), b.to(dtype), padding=1), slope)


def lateral_ref(x, w, b, up, dtype, slope=0.1):
    y = lrelu(torch.nn.functional.conv2d(x.to(dtype), w.to(dtype), b.to(dtype)), slope)
    return y if up is None else y + nearest(up.to(dtype), y.shape[2], y.shape[3])


def heads_ref(x, w, b, dtype):
    """w (32, 64, 1, 1): class (4), box (8), landmark (20) channels -> the permute / view of the heads: (B, 2 H W, 2 | 4 | 10)"""
    y = torch.nn.functional.conv2d(x.to(dtype), w.to(dtype), b.to(dtype)).permute(0, 2, 3, 1).contiguous()
    B = y.shape[0]
    return y[..., 0:4].reshape(B, -1, 2), y[..., 4:12].reshape(B, -1, 4), y[..., 12:32].reshape(B, -1, 10)


def folded_forward(folded, x):
    """The whole network from detect.fold_state's dictionary (the kernels' layouts), in x's dtype -> (conf, loc, lm)"""
    dt = x.dtype

    def dense(name):
        w = folded[name + ".w"]
        return w.reshape(w.shape[0], 3, 3, w.shape[2]).permute(3, 0, 1, 2), folded[name + ".b"]

    def point(name):
        w = folded[name + ".w"]
        return w.t().reshape(w.shape[1], w.shape[0], 1, 1), folded[name + ".b"]

    def depth(name):
        w = folded[name + ".w"]
        return w.reshape(w.shape[0], 1, 3, 3), folded[name + ".b"]
    F = torch.nn.functional
    w, b = dense("body.stage1.0.0")
    x = lrelu(F.conv2d(x, w.to(dt), b.to(dt), stride=2, padding=1), 0.1)
    feats = []
    for stage, strides in (("stage1", (None, 1, 2, 1, 2, 1)), ("stage2", (2, 1, 1, 1, 1, 1)), ("stage3", (2, 1))):
        for k, s in enumerate(strides):
            if s is not None:
                x = sep_ref(x, *depth(f"body.{stage}.{k}.0"), *point(f"body.{stage}.{k}.3"), s, dt)
        feats.append(x)
    o3 = lateral_ref(feats[2], *point("fpn.output3.0"), None, dt)
    o2 = conv3x3_ref(lateral_ref(feats[1], *point("fpn.output2.0"), o3, dt), *dense("fpn.merge2.0"), 0.1, dt)
    o1 = conv3x3_ref(lateral_ref(feats[0], *point("fpn.output1.0"), o2, dt), *dense("fpn.merge1.0"), 0.1, dt)
    outs = []
    for k, f in enumerate((o1, o2, o3)):
        q = f"ssh{k + 1}."
        t = conv3x3_ref(f, *dense(q + "conv5X5_1.0"), 0.1, dt)
        s = torch.relu(torch.cat([conv3x3_ref(f, *dense(q + "conv3X3.0"), None, dt), conv3x3_ref(t, *dense(q + "conv5X5_2.0"), None, dt),
                                  conv3x3_ref(conv3x3_ref(t, *dense(q + "conv7X7_2.0"), 0.1, dt), *dense(q + "conv7x7_3.0"), None, dt)], dim=1))
        hw = folded[f"heads.{k}.w"]
        outs.append(heads_ref(s, hw.t().reshape(32, 64, 1, 1), folded[f"heads.{k}.b"], dt))
    return tuple(torch.cat([o[i] for o in outs], dim=1) for i in range(3))
