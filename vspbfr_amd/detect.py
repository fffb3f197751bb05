"""Face detection for whole photos: RetinaFace with the MobileNet-0.25 backbone on the device, the host side of csrc/detect.hip.
A checkpoint of the ResNet-50 network goes to vspbfr_amd.detect_r50: load_detector chooses by key.

    python -m vspbfr_amd.detect --photos DIR --weights W --out landmarks.json [--threshold 0.8] [--nms 0.4] [--side 1024]
        [--max_faces N] [--min_face PX]

writes the file `python -m vspbfr_amd.restore_photos --landmarks` reads: {"relative/name.png": [[[x, y] x 5], ...one entry per face]},
five landmarks in photo pixels (pixel centres) in the order of photo.FFHQ512_TEMPLATE.  Every float is written with the shortest
digits that give back its float32 value.

    expected_state / check_state_dict   the key layout of the public `mobilenet0.25` RetinaFace checkpoint (300 entries) and the loader's rules
    fold_state                          BatchNorm folded into weight and bias in float64, in the kernels' layouts
    RetinaFaceDetector                  weights -> network(), postprocess(), detect()
    load_detector                       a file with `body.layer1.0.conv1.weight` -> detect_r50.RetinaFaceR50Detector, any other -> RetinaFaceDetector
    write_landmarks / format_f32        the JSON writer

No weights are shipped.  The key layout is written from the public model definition and could not be checked against a real checkpoint
file; a file that deviates is refused by key name, never half-loaded.

The canvas of one detect() call: photo k is scaled by s = min(1, side / max(h, w)) -- through the ragged device LANCZOS resize
(resample.ResamplePlan) where s < 1, read in place where s = 1 -- and lies at the top-left of image k of a (B, Hc, Wc) batch, Hc and Wc
the group's largest resized sides rounded up to 32; the rest holds the mean colour.  Network coordinates have pixel k spanning
[k, k + 1); detections come back as x_photo = x_canvas (w / w_resized) - 0.5, this repository's pixel-centre convention."""
import argparse
import json
import os

import numpy as np
import torch

MEAN_BGR = (104.0, 117.0, 123.0)
STEPS = (8, 16, 32)
MIN_SIZES = ((16, 32), (64, 128), (256, 512))
DEFAULT_SIDE, DEFAULT_THRESHOLD, DEFAULT_NMS, DEFAULT_MAX_CANDIDATES, DEFAULT_MAX_FACES = 1024, 0.8, 0.4, 1024, 256
BN_EPS = 1e-5
BN_KEYS = ("weight", "bias", "running_mean", "running_var")

# (name, [(cin, cout, stride), ...]) of the backbone: block 0 of stage1 is the dense entry, every other block is depthwise-separable
STAGES = (("stage1", [(3, 8, 2), (8, 16, 1), (16, 32, 2), (32, 32, 1), (32, 64, 2), (64, 64, 1)]),
          ("stage2", [(64, 128, 2)] + [(128, 128, 1)] * 5),
          ("stage3", [(128, 256, 2), (256, 256, 1)]))
SSH = (("conv3X3", 64, 32), ("conv5X5_1", 64, 16), ("conv5X5_2", 16, 16), ("conv7X7_2", 16, 16), ("conv7x7_3", 16, 16))
HEADS = (("ClassHead", 4), ("BboxHead", 8), ("LandmarkHead", 20))


def conv_units():
    """[(prefix of the conv, prefix of its BatchNorm, weight shape)] of every conv + BN pair, in checkpoint order"""
    units = []
    for stage, blocks in STAGES:
        for k, (ci, co, _) in enumerate(blocks):
            p = f"body.{stage}.{k}"
            if ci == 3:
                units.append((f"{p}.0", f"{p}.1", (co, ci, 3, 3)))
            else:
                units.append((f"{p}.0", f"{p}.1", (ci, 1, 3, 3)))
                units.append((f"{p}.3", f"{p}.4", (co, ci, 1, 1)))
    for k, ci in ((1, 64), (2, 128), (3, 256)):
        units.append((f"fpn.output{k}.0", f"fpn.output{k}.1", (64, ci, 1, 1)))
    for k in (1, 2):
        units.append((f"fpn.merge{k}.0", f"fpn.merge{k}.1", (64, 64, 3, 3)))
    for k in (1, 2, 3):
        for name, ci, co in SSH:
            units.append((f"ssh{k}.{name}.0", f"ssh{k}.{name}.1", (co, ci, 3, 3)))
    return units


def expected_state(with_tracked=True):
    """{key: shape} of the checkpoint: 47 conv + BN pairs and nine 1x1 heads, 300 entries with the BatchNorm counters"""
    out = {}
    for conv, bn, shape in conv_units():
        out[conv + ".weight"] = shape
        for k in BN_KEYS:
            out[f"{bn}.{k}"] = (shape[0],)
        if with_tracked:
            out[bn + ".num_batches_tracked"] = ()
    for head, n in HEADS:
        for k in range(3):
            out[f"{head}.{k}.conv1x1.weight"] = (n, 64, 1, 1)
            out[f"{head}.{k}.conv1x1.bias"] = (n,)
    return out


def check_state_dict(sd, want=None, what="RetinaFace mobilenet0.25 checkpoint"):
    """The loader's rules: a leading `module.` is stripped from every key, `num_batches_tracked` entries are ignored, any other missing or
    unexpected key and any wrong shape is a ValueError that names it -> {key: float64 CPU tensor}.  want: {key: shape} without the
    BatchNorm counters (this module's expected_state by default), `what` the name of the checkpoint in the messages."""
    if isinstance(sd, dict) and "state_dict" in sd and not any(str(k).endswith(".weight") for k in sd):
        sd = sd["state_dict"]
    clean = {}
    for k, v in sd.items():
        k = k[len("module."):] if k.startswith("module.") else k
        if not k.endswith("num_batches_tracked"):
            clean[k] = v
    want = expected_state(with_tracked=False) if want is None else want
    missing, extra = sorted(set(want) - set(clean)), sorted(set(clean) - set(want))
    if missing or extra:
        raise ValueError(what + ": " + "; ".join(
            f"{what} {', '.join(ks[:8])}{' ...' if len(ks) > 8 else ''}" for what, ks in (("missing keys", missing), ("unexpected keys", extra)) if ks))
    out = {}
    for k, shape in want.items():
        t = torch.as_tensor(clean[k]).detach().to("cpu", torch.float64)
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{what}: {k} has shape {tuple(t.shape)}, expected {tuple(shape)}")
        out[k] = t
    return out


def fold_bn(sd, conv, bn):
    """(weight, bias) in float64 of conv + BatchNorm (eval): w g / sqrt(var + eps), beta - mean g / sqrt(var + eps)"""
    g = sd[bn + ".weight"] / torch.sqrt(sd[bn + ".running_var"] + BN_EPS)
    return sd[conv + ".weight"] * g.view(-1, 1, 1, 1), sd[bn + ".bias"] - sd[bn + ".running_mean"] * g


def pack_dense(w):
    """(Cout, Cin, 3, 3) -> (Cin, 9, Cout), the layout of vsp_det_conv3x3_f32 (and, for Cin = 3, of vsp_det_entry_u8)"""
    return w.permute(1, 2, 3, 0).reshape(w.shape[1], 9, w.shape[0]).contiguous()


def pack_pointwise(w):
    """(Cout, Cin, 1, 1) -> (Cin, Cout)"""
    return w.reshape(w.shape[0], w.shape[1]).t().contiguous()


def pack_depthwise(w):
    """(C, 1, 3, 3) -> (C, 9)"""
    return w.reshape(w.shape[0], 9).contiguous()


def fold_state(sd):
    """Checked state dict -> {name: float64 tensor} in the kernels' layouts: `<conv prefix>.w` / `.b` for every conv + BN pair (packed by
    kind) and `heads.<k>.w` (64, 32) / `.b` (32) with the class, box and landmark heads of level k side by side"""
    out = {}
    for conv, bn, shape in conv_units():
        w, b = fold_bn(sd, conv, bn)
        if shape[2] == 1:
            w = pack_pointwise(w)
        elif shape[1] == 1:
            w = pack_depthwise(w)
        else:
            w = pack_dense(w)
        out[conv + ".w"], out[conv + ".b"] = w, b
    for k in range(3):
        out[f"heads.{k}.w"] = pack_pointwise(torch.cat([sd[f"{h}.{k}.conv1x1.weight"] for h, _ in HEADS]))
        out[f"heads.{k}.b"] = torch.cat([sd[f"{h}.{k}.conv1x1.bias"] for h, _ in HEADS])
    return out


def level_sizes(Hc, Wc):
    """[(H, W)] of the three feature maps of an (Hc, Wc) canvas: ceil(Hc / step)"""
    return [(-(-Hc // s), -(-Wc // s)) for s in STEPS]


def num_priors(Hc, Wc):
    return sum(2 * h * w for h, w in level_sizes(Hc, Wc))


def resized_size(h, w, side):
    """(scale, h', w') of a photo for a canvas of at most `side`: s = min(1, side / max(h, w)), sizes rounded half up, at least 1"""
    s = min(1.0, float(side) / float(max(h, w)))
    if s >= 1.0:
        return 1.0, int(h), int(w)
    return s, max(1, int(h * s + 0.5)), max(1, int(w * s + 0.5))


def format_f32(v):
    """the shortest decimal string that gives back the float32 value v"""
    v = np.float32(v)
    if not np.isfinite(v):
        raise ValueError(f"format_f32: {v}")
    return np.format_float_positional(v, unique=True, trim="0")


def as_json_floats(a):
    """float32 values -> the float64 values a file written by write_landmarks gives back (the same array shape)"""
    a = np.asarray(a, dtype=np.float32)
    return np.array([float(format_f32(v)) for v in a.reshape(-1)], dtype=np.float64).reshape(a.shape)


def landmarks_json(faces_by_name):
    """{name: [(5, 2) array, ...]} -> the text of a --landmarks file, floats through format_f32"""
    lines = []
    for name, faces in faces_by_name.items():
        body = ", ".join("[" + ", ".join(f"[{format_f32(x)}, {format_f32(y)}]" for x, y in np.asarray(f).reshape(5, 2)) + "]" for f in faces)
        lines.append(f" {json.dumps(name)}: [{body}]")
    return "{\n" + ",\n".join(lines) + "\n}\n"


def write_landmarks(path, faces_by_name):
    with open(path, "w") as f:
        f.write(landmarks_json(faces_by_name))


class RetinaFaceDetector:
    """weights: a path (torch.load) or a state dict in the `mobilenet0.25` RetinaFace layout -> the detector on `device`.  BatchNorm is
    folded once, here, in float64; the kernels run in fp32.  There is no fallback: a layer the kernels refuse raises."""

    def __init__(self, weights, device):
        if isinstance(weights, (str, os.PathLike)):
            weights = torch.load(weights, map_location="cpu")
        self.device = torch.device(device)
        self.folded = fold_state(check_state_dict(weights))
        self.p = {k: v.to(torch.float32).contiguous().to(self.device) for k, v in self.folded.items()}
        self.device = self.p["heads.0.b"].device               # with its index

    # ------------------------------------------------------------------------------------------------------------------- network
    def network(self, sources, B, Hc, Wc):
        """sources: [(flat uint8 device buffer, [(byte offset, h, w, slot), ...]), ...] that together fill slots 0 .. B - 1 of the
        canvas batch -> (conf (B, P, 2), loc (B, P, 4), lm (B, P, 10)) on the device"""
        from . import _lib, hip_ops as H
        p = self.p
        x = torch.empty((B, 8, (Hc + 1) // 2, (Wc + 1) // 2), device=self.device, dtype=torch.float32)
        slots = sorted(s for _, items in sources for *_, s in items)
        if slots != list(range(B)):
            raise ValueError(f"RetinaFaceDetector.network: the sources fill slots {slots}, not 0..{B - 1}")
        for buf, items in sources:
            if not items:
                continue
            tab = (_lib.DetSrc * len(items))()
            for t, (off, h, w, slot) in zip(tab, items):
                t.off, t.h, t.w, t.slot = int(off), int(h), int(w), int(slot)
            tab_dev = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(self.device)
            H.det_entry_u8(x, buf, tab, tab_dev, len(items), p["body.stage1.0.0.w"], p["body.stage1.0.0.b"], Hc, Wc)
        feats = []
        for stage, blocks in STAGES:
            for k, (ci, co, stride) in enumerate(blocks):
                if ci == 3:
                    continue
                q = f"body.{stage}.{k}"
                x = H.det_sep(x, p[q + ".0.w"], p[q + ".0.b"], p[q + ".3.w"], p[q + ".3.b"], stride)
            feats.append(x)
        a, b, c = feats
        o3 = H.det_lateral(c, p["fpn.output3.0.w"], p["fpn.output3.0.b"])
        o2 = H.det_conv3x3(H.det_lateral(b, p["fpn.output2.0.w"], p["fpn.output2.0.b"], up=o3), p["fpn.merge2.0.w"], p["fpn.merge2.0.b"], 0.1)
        o1 = H.det_conv3x3(H.det_lateral(a, p["fpn.output1.0.w"], p["fpn.output1.0.b"], up=o2), p["fpn.merge1.0.w"], p["fpn.merge1.0.b"], 0.1)
        P = num_priors(Hc, Wc)
        conf = torch.empty((B, P, 2), device=self.device, dtype=torch.float32)
        loc = torch.empty((B, P, 4), device=self.device, dtype=torch.float32)
        lm = torch.empty((B, P, 10), device=self.device, dtype=torch.float32)
        p0 = 0
        for k, f in enumerate((o1, o2, o3)):
            H.det_heads(self.ssh(k + 1, f), p[f"heads.{k}.w"], p[f"heads.{k}.b"], conf, loc, lm, p0)
            p0 += 2 * f.shape[2] * f.shape[3]
        return conf, loc, lm

    def ssh(self, k, x):
        """relu(cat[conv3X3(x), conv5X5_2(t), conv7x7_3(conv7X7_2(t))]), t = conv5X5_1(x): the three branches write their channel windows"""
        from . import hip_ops as H
        p = self.p

        def wb(name):
            return p[f"ssh{k}.{name}.0.w"], p[f"ssh{k}.{name}.0.b"]
        out = torch.empty((x.shape[0], 64, x.shape[2], x.shape[3]), device=x.device, dtype=torch.float32)
        H.det_conv3x3(x, *wb("conv3X3"), 0.0, out=out, y_coff=0)
        t = H.det_conv3x3(x, *wb("conv5X5_1"), 0.1)
        H.det_conv3x3(t, *wb("conv5X5_2"), 0.0, out=out, y_coff=32)
        H.det_conv3x3(H.det_conv3x3(t, *wb("conv7X7_2"), 0.1), *wb("conv7x7_3"), 0.0, out=out, y_coff=48)
        return out

    # ----------------------------------------------------------------------------------------------------------- post-processing
    @staticmethod
    def postprocess(conf, loc, lm, Hc, Wc, threshold=DEFAULT_THRESHOLD, nms=DEFAULT_NMS, max_candidates=DEFAULT_MAX_CANDIDATES,
                    max_faces=DEFAULT_MAX_FACES):
        """vsp_det_decode_nms_f32 -> per image a dict: box (n, 4), score (n,), lm (n, 10) float32 in canvas pixels, prior (n,) int32,
        status, candidates, nonfinite.  One read of the device."""
        from . import hip_ops as H
        faces, info = H.det_decode_nms(conf, loc, lm, Hc, Wc, threshold, nms, max_candidates, max_faces)
        faces, info = faces.cpu().numpy(), info.cpu().numpy()
        out = []
        for b in range(faces.shape[0]):
            n = int(info[b, 0])
            rec = faces[b, :n].reshape(n, 64)
            f = rec.view(np.float32).reshape(n, 16)
            out.append({"box": f[:, 0:4].copy(), "score": f[:, 4].copy(), "lm": f[:, 5:15].copy(), "prior": rec.view(np.int32).reshape(n, 16)[:, 15].copy(),
                        "status": int(info[b, 1]), "candidates": int(info[b, 2]), "nonfinite": int(info[b, 3])})
        return out

    # -------------------------------------------------------------------------------------------------------------------- canvas
    def canvas(self, photos=None, device_photos=None, side=DEFAULT_SIDE):
        """The sources of network() for one group of photos -> (sources, B, Hc, Wc, [(h, w, h', w'), ...]).  photos: uint8 (h, w, 3)
        arrays; device_photos = (flat uint8 device buffer, byte offsets, [(h, w), ...]) as jpeg.decode_files returns them."""
        if (photos is None) == (device_photos is None):
            raise ValueError("detect: give photos or device_photos")
        if int(side) < 32:
            raise ValueError(f"detect: side {side}")
        if photos is not None:
            arrs = []
            for k, a in enumerate(photos):
                a = np.asarray(a)
                if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
                    raise ValueError(f"detect: photo {k} must be uint8 (h, w, 3), got {a.dtype} {a.shape}")
                arrs.append(np.ascontiguousarray(a).reshape(-1))
            sizes = [np.asarray(a).shape[:2] for a in photos]
            offsets = np.concatenate([[0], np.cumsum([a.size for a in arrs])])[:-1].tolist() if arrs else []
            buffer = torch.from_numpy(np.concatenate(arrs)).to(self.device) if arrs else torch.empty(0, dtype=torch.uint8, device=self.device)
        else:
            buffer, offsets, sizes = device_photos
            if buffer.dtype != torch.uint8 or buffer.dim() != 1 or not buffer.is_contiguous() or buffer.device != self.device:
                raise ValueError(f"detect: device_photos takes a flat contiguous uint8 tensor on {self.device}")
        sizes = [(int(h), int(w)) for h, w in sizes]
        if not sizes or len(offsets) != len(sizes):
            raise ValueError("detect: at least one photo, one byte offset per photo")
        geo = [(h, w) + resized_size(h, w, side)[1:] for h, w in sizes]
        Hc = -(-max(g[2] for g in geo) // 32) * 32
        Wc = -(-max(g[3] for g in geo) // 32) * 32
        small = [k for k, g in enumerate(geo) if g[:2] != g[2:]]
        sources = [(buffer, [(offsets[k], geo[k][0], geo[k][1], k) for k in range(len(geo)) if k not in small])]
        if small:
            from .resample import ResamplePlan
            plan = ResamplePlan([geo[k][:2] for k in small], [(geo[k][3], geo[k][2]) for k in small], [(0, 0)] * len(small), None,
                                device_sources=(buffer, [offsets[k] for k in small]), out_sizes=[geo[k][2:] for k in small])
            out = plan.run_into(torch.empty(plan.out_bytes, dtype=torch.uint8, device=self.device))
            sources.append((out, [(plan.out_offsets[i], geo[k][2], geo[k][3], k) for i, k in enumerate(small)]))
        return sources, len(geo), Hc, Wc, geo

    def detect(self, photos=None, device_photos=None, side=DEFAULT_SIDE, threshold=DEFAULT_THRESHOLD, nms=DEFAULT_NMS,
               max_faces=DEFAULT_MAX_FACES, max_candidates=DEFAULT_MAX_CANDIDATES, min_face=0.0):
        """-> per photo a dict: landmarks (n, 5, 2), box (n, 4), score (n,) float32 in photo pixels (pixel centres), best score first,
        prior (n,), status, candidates, nonfinite, canvas = (Hc, Wc), resized = (h', w').  min_face: faces whose box is narrower or
        lower than this many photo pixels are left out."""
        sources, B, Hc, Wc, geo = self.canvas(photos, device_photos, side)
        conf, loc, lm = self.network(sources, B, Hc, Wc)
        out = self.postprocess(conf, loc, lm, Hc, Wc, threshold, nms, max_candidates, max_faces)
        for d, (h, w, hr, wr) in zip(out, geo):
            sx, sy = np.float64(w) / wr, np.float64(h) / hr
            sc = np.array([sx, sy], dtype=np.float64)
            box = (d["box"].astype(np.float64).reshape(-1, 2, 2) * sc - 0.5).reshape(-1, 4)
            pts = d.pop("lm").astype(np.float64).reshape(-1, 5, 2) * sc - 0.5
            keep = np.minimum(box[:, 2] - box[:, 0], box[:, 3] - box[:, 1]) >= float(min_face)
            d.update(box=box[keep].astype(np.float32), landmarks=pts[keep].astype(np.float32), score=d["score"][keep], prior=d["prior"][keep],
                     canvas=(Hc, Wc), resized=(hr, wr))
        return out


def load_detector(weights, device):
    """weights: a path (torch.load) or a state dict -> the detector for it: a checkpoint that holds `body.layer1.0.conv1.weight` (after the
    loader's `module.` stripping) is RetinaFace's ResNet-50 network and goes to detect_r50.RetinaFaceR50Detector, anything else to
    RetinaFaceDetector, whose loader accepts or refuses it as before."""
    if isinstance(weights, (str, os.PathLike)):
        weights = torch.load(weights, map_location="cpu")
    sd = weights
    if isinstance(sd, dict) and "state_dict" in sd and not any(str(k).endswith(".weight") for k in sd):
        sd = sd["state_dict"]
    if isinstance(sd, dict) and any(str(k) in ("body.layer1.0.conv1.weight", "module.body.layer1.0.conv1.weight") for k in sd):
        from .detect_r50 import RetinaFaceR50Detector
        return RetinaFaceR50Detector(weights, device)
    return RetinaFaceDetector(weights, device)


def add_detect_arguments(ap, prefix=""):
    """the five detection options of both CLIs (`prefix` = "detect_" in restore_photos)"""
    ap.add_argument(f"--{prefix}threshold", type=float, default=DEFAULT_THRESHOLD, help="score above which a prior is a candidate")
    ap.add_argument(f"--{prefix}nms", type=float, default=DEFAULT_NMS, help="IoU above which a candidate is suppressed by a kept one")
    ap.add_argument(f"--{prefix}side", type=int, default=DEFAULT_SIDE, help="photos larger than this are shrunk to it for detection")
    ap.add_argument(f"--{prefix}max_faces", type=int, default=DEFAULT_MAX_FACES, help="faces kept per photo, best score first")
    ap.add_argument(f"--{prefix}min_face", type=float, default=0.0, help="faces whose box is smaller than this many photo pixels are left out")


def check_detect_arguments(threshold, nms, side, max_faces, min_face):
    """ValueError for an option outside its range (before any model is loaded)"""
    if not 0.0 <= threshold < 1.0:
        raise ValueError(f"detection threshold {threshold} outside [0, 1)")
    if not 0.0 <= nms <= 1.0:
        raise ValueError(f"detection nms {nms} outside [0, 1]")
    if not 32 <= side <= 8192:
        raise ValueError(f"detection side {side} outside 32..8192")
    if max_faces < 1:
        raise ValueError(f"detection max_faces {max_faces} must be at least 1")
    if not min_face >= 0.0:
        raise ValueError(f"detection min_face {min_face} must be at least 0")
    return dict(threshold=float(threshold), nms=float(nms), side=int(side), max_faces=int(max_faces), min_face=float(min_face))


def main(argv=None):
    ap = argparse.ArgumentParser(description="Detect faces in photos and write the landmarks file of vspbfr_amd.restore_photos")
    ap.add_argument("--photos", type=str, required=True, help="directory of photos (searched recursively)")
    ap.add_argument("--weights", type=str, required=True, help="RetinaFace checkpoint, mobilenet0.25 or resnet50 (not shipped)")
    ap.add_argument("--out", type=str, required=True, help="the landmarks JSON to write")
    add_detect_arguments(ap)
    args = ap.parse_args(argv)
    try:
        params = check_detect_arguments(args.threshold, args.nms, args.side, args.max_faces, args.min_face)
        from .restore_photos import MAX_PHOTOS_PER_CALL, _decode, list_photos
        names = list_photos(args.photos)
        if not os.path.isfile(args.weights):
            raise ValueError(f"--weights: no such file: {args.weights}")
    except (ValueError, OSError) as e:
        ap.error(str(e))
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(device)
    try:
        det = load_detector(args.weights, device)
    except ValueError as e:
        ap.error(str(e))
    found = {}
    for i in range(0, len(names), MAX_PHOTOS_PER_CALL):
        group = names[i:i + MAX_PHOTOS_PER_CALL]
        res = det.detect(photos=[_decode(os.path.join(args.photos, n)) for n in group], **params)
        for n, d in zip(group, res):
            if len(d["landmarks"]):
                found[n] = list(d["landmarks"])
            print(f"{n}: {len(d['landmarks'])} faces" + (f" (status {d['status']})" if d["status"] else ""))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    write_landmarks(args.out, found)


if __name__ == "__main__":
    main()
