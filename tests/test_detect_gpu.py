"""GPU: the detector's kernels (csrc/detect.hip) against the float64 restatement of tests/detect_ref.py.

    max|HIP - float64| <= 4 * e_ref + 2e-6 * max|float64|,     e_ref = max|fp32 CPU evaluation - float64| on the same operands

-- the bound of tests/test_tacc_kernels.py; nothing in it comes from the kernels.  Every comparison prints e_ref, the HIP error and their
ratio (`pytest -s`).  Orders and sets (kept priors, status words) are compared exactly."""
import ctypes as C

import numpy as np
import pytest
import torch

import detect_cases as K
import detect_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def close(got, r64, r32, what, scale=1.0):
    got, r64, r32 = (np.asarray(t.detach().cpu() if isinstance(t, torch.Tensor) else t, dtype=np.float64) for t in (got, r64, r32))
    assert got.shape == r64.shape, (what, got.shape, r64.shape)
    eref = float(np.abs(r32 - r64).max()) if r64.size else 0.0
    err = float(np.abs(got - r64).max()) if r64.size else 0.0
    tol = (4.0 * eref + 2e-6 * (float(np.abs(r64).max()) if r64.size else 0.0)) * scale
    print(f"DET {what}: e_ref={eref:.3e} e_hip={err:.3e} ratio={err / eref if eref else float('nan'):.2f} tol={tol:.3e}")
    assert err <= tol, f"{what}: max|d|={err:.3e} tol={tol:.3e} (e_ref {eref:.3e})"


def rand(gen, *shape, scale=1.0):
    return torch.randn(*shape, generator=gen, dtype=torch.float64).mul_(scale).float()      # fp32 values: the same operands everywhere


@pytest.fixture(scope="module")
def detector():
    from vspbfr_amd.detect import RetinaFaceDetector
    return RetinaFaceDetector(K.model().state_dict(), DEV)


@pytest.mark.parametrize("cin,cout,stride,hw", [(8, 16, 1, (13, 17)), (16, 32, 2, (13, 17)), (128, 128, 1, (13, 17)), (128, 256, 2, (5, 7))])
def test_separable_block(cin, cout, stride, hw):
    from vspbfr_amd import detect as D, hip_ops as H
    g = torch.Generator().manual_seed(cin + cout)
    x = rand(g, 2, cin, *hw)
    wd, bd = rand(g, cin, 1, 3, 3, scale=1 / 3), rand(g, cin, scale=0.1)
    wp, bp = rand(g, cout, cin, 1, 1, scale=cin ** -0.5), rand(g, cout, scale=0.1)
    y = H.det_sep(x.to(DEV), D.pack_depthwise(wd).to(DEV), bd.to(DEV), D.pack_pointwise(wp).to(DEV), bp.to(DEV), stride)
    assert tuple(y.shape) == (2, cout, (hw[0] - 1) // stride + 1, (hw[1] - 1) // stride + 1)
    close(y, R.sep_ref(x, wd, bd, wp, bp, stride, torch.float64), R.sep_ref(x, wd, bd, wp, bp, stride, torch.float32), f"sep {cin}->{cout} s{stride} {hw}")


def test_entry_kernel_places_photos_at_the_top_left_of_a_padded_canvas():
    from vspbfr_amd import _lib, detect as D, hip_ops as H
    g = torch.Generator().manual_seed(11)
    photos = [R.test_photo(37, 45, 1), R.test_photo(64, 20, 2)]
    w, b = rand(g, 8, 3, 3, 3, scale=27 ** -0.5 / 64), rand(g, 8, scale=0.1)
    flat = np.concatenate([p.reshape(-1) for p in photos])
    tab = (_lib.DetSrc * 2)()
    tab[0].off, tab[0].h, tab[0].w, tab[0].slot = 0, 37, 45, 1            # the slots are swapped: item order is not canvas order
    tab[1].off, tab[1].h, tab[1].w, tab[1].slot = 37 * 45 * 3, 64, 20, 0
    tab_dev = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(DEV)
    y = torch.full((2, 8, 32, 32), float("nan"), device=DEV)
    H.det_entry_u8(y, torch.from_numpy(flat).to(DEV), tab, tab_dev, 2, D.pack_dense(w).to(DEV), b.to(DEV), 64, 64)
    order = [photos[1], photos[0]]
    close(y, R.entry_ref(order, 64, 64, w, b, torch.float64), R.entry_ref(order, 64, 64, w, b, torch.float32), "entry 37x45 + 64x20 in 64x64")


@pytest.mark.parametrize("cin,cout,slope", [(64, 64, 0.1), (64, 32, None), (16, 16, 0.0)])
def test_dense_3x3(cin, cout, slope):
    from vspbfr_amd import detect as D, hip_ops as H
    g = torch.Generator().manual_seed(cin * cout)
    x, w, b = rand(g, 2, cin, 13, 17), rand(g, cout, cin, 3, 3, scale=(9 * cin) ** -0.5), rand(g, cout, scale=0.1)
    out = torch.full((2, cout + 24, 13, 17), 7.0, device=DEV)
    H.det_conv3x3(x.to(DEV), D.pack_dense(w).to(DEV), b.to(DEV), slope, out=out, y_coff=16)
    assert bool((out[:, :16] == 7.0).all()) and bool((out[:, 16 + cout:] == 7.0).all())          # the channel window alone is written
    close(out[:, 16:16 + cout], R.conv3x3_ref(x, w, b, slope, torch.float64), R.conv3x3_ref(x, w, b, slope, torch.float32), f"conv3x3 {cin}->{cout} slope {slope}")
    y = H.det_conv3x3(x.to(DEV), D.pack_dense(w).to(DEV), b.to(DEV), slope)
    assert torch.equal(y, out[:, 16:16 + cout])


@pytest.mark.parametrize("cin,hw,hw2", [(128, (13, 17), (7, 9)), (256, (7, 9), (4, 5)), (256, (4, 5), None)])
def test_lateral_with_upsample_add(cin, hw, hw2):
    from vspbfr_amd import detect as D, hip_ops as H
    g = torch.Generator().manual_seed(cin + hw[0])
    x, w, b = rand(g, 2, cin, *hw), rand(g, 64, cin, 1, 1, scale=cin ** -0.5), rand(g, 64, scale=0.1)
    up = None if hw2 is None else rand(g, 2, 64, *hw2)
    y = H.det_lateral(x.to(DEV), D.pack_pointwise(w).to(DEV), b.to(DEV), None if up is None else up.to(DEV))
    close(y, R.lateral_ref(x, w, b, up, torch.float64), R.lateral_ref(x, w, b, up, torch.float32), f"lateral {cin} {hw} <- {hw2}")


def test_heads_write_the_prior_layout():
    from vspbfr_amd import detect as D, hip_ops as H
    g = torch.Generator().manual_seed(5)
    levels, P = [(13, 17), (7, 9), (4, 5)], 2 * (13 * 17 + 7 * 9 + 4 * 5)
    conf, loc, lm = (torch.full((2, P, n), float("nan"), device=DEV) for n in (2, 4, 10))
    want64, want32, p0 = [], [], 0
    for h, w_ in levels:
        x, w, b = rand(g, 2, 64, h, w_), rand(g, 32, 64, 1, 1, scale=1 / 8), rand(g, 32, scale=0.3)
        H.det_heads(x.to(DEV), D.pack_pointwise(w).to(DEV), b.to(DEV), conf, loc, lm, p0)
        p0 += 2 * h * w_
        want64.append(R.heads_ref(x, w, b, torch.float64))
        want32.append(R.heads_ref(x, w, b, torch.float32))
    for i, (got, name) in enumerate(((conf, "conf"), (loc, "loc"), (lm, "lm"))):
        close(got, torch.cat([t[i] for t in want64], dim=1), torch.cat([t[i] for t in want32], dim=1), f"heads {name}")


def test_whole_network(detector):
    case = K.detection_case()
    sources, B, Hc, Wc, _ = detector.canvas(photos=case["canvas_photos"], side=K.SIDE)
    assert (B, Hc, Wc) == (2, K.HC, K.WC)
    out = detector.network(sources, B, Hc, Wc)
    for got, r64, r32, name in zip(out, case["o64"], case["o32"], ("conf", "loc", "lm")):
        close(got, r64, r32, f"network {name}")


def _faces(d):
    return d["prior"].astype(np.int64)


@pytest.mark.parametrize("caps", [(1024, 256), (64, 4)])
def test_post_processing_on_synthetic_heads(detector, caps):
    conf, loc, lm = K.synthetic_heads()
    got = detector.postprocess(*(torch.from_numpy(a).to(DEV) for a in (conf, loc, lm)), K.HC, K.WC, K.THRESHOLD, K.NMS, *caps)
    for k in range(3):
        d64, d32 = (R.decode(conf[k], loc[k], lm[k], K.HC, K.WC, dt) for dt in (np.float64, np.float32))
        r = R.select_nms(*d64, K.THRESHOLD, K.NMS, *caps)
        print(f"image {k} caps {caps}: {r['candidates']} candidates, kept {len(r['keep'])}, status {r['status']}; HIP kept {len(got[k]['prior'])}, status {got[k]['status']}")
        assert list(_faces(got[k])) == list(r["keep"])
        assert (got[k]["status"], got[k]["candidates"], got[k]["nonfinite"]) == (r["status"], r["candidates"], r["nonfinite"])
        keep = r["keep"]
        close(got[k]["score"], d64[0][keep], d32[0][keep], f"nms score image {k}")
        close(got[k]["box"], d64[1][keep], d32[1][keep], f"nms box image {k}")
        close(got[k]["lm"], d64[2][keep], d32[2][keep], f"nms landmarks image {k}")
    assert len(got[2]["prior"]) == 0 and got[2]["status"] == 0
    if caps == (64, 4):
        assert got[1]["status"] == R.CAND_CAPPED | R.FACES_CAPPED and len(got[1]["prior"]) == 4


def test_post_processing_drops_and_counts_non_finite_candidates(detector):
    conf, loc, lm = (a.copy() for a in K.synthetic_heads())
    n0 = 2 * 12 * 16
    p = [n0 + 2 * (1 * 8 + 1), n0 + 2 * (3 * 8 + 5) + 1]            # two planted candidates of image 0
    loc[0, p[0], 2] = 4000.0                                         # exp overflows at either precision: an infinite box
    lm[0, p[1], 3] = np.nan
    got = detector.postprocess(*(torch.from_numpy(a).to(DEV) for a in (conf, loc, lm)), K.HC, K.WC, K.THRESHOLD, K.NMS)[0]
    r = R.select_nms(*R.decode(conf[0], loc[0], lm[0], K.HC, K.WC), K.THRESHOLD, K.NMS)
    assert r["nonfinite"] == 2 and r["status"] == R.NONFINITE
    assert list(_faces(got)) == list(r["keep"]) and (got["status"], got["candidates"], got["nonfinite"]) == (r["status"], r["candidates"], 2)
    assert not set(p) & set(_faces(got))


def test_detect_end_to_end(detector):
    case = K.detection_case()
    res = detector.detect(photos=case["photos"], side=K.SIDE, threshold=K.THRESHOLD, nms=K.NMS)
    for k, (d, (h, w, hr, wr)) in enumerate(zip(res, case["geo"])):
        ref = case["det"][k]
        keep = ref["r64"]["keep"]
        assert d["canvas"] == (K.HC, K.WC) and d["resized"] == (hr, wr)
        assert list(_faces(d)) == list(keep) and d["status"] == ref["r64"]["status"] == 0
        close(d["score"], ref["d64"][0][keep], ref["d32"][0][keep], f"detect score photo {k}")
        # the bound on canvas coordinates, scaled into the photo with them
        sc = max(w / wr, h / hr)
        for name, col in (("landmarks", 2), ("box", 1)):
            c64, c32 = ref["d64"][col][keep], ref["d32"][col][keep]
            eref = float(np.abs(c32.astype(np.float64) - c64).max())
            tol = (4.0 * eref + 2e-6 * float(np.abs(c64).max())) * sc
            want = R.to_photo(c64.reshape(len(keep), -1, 2), h, w, hr, wr)
            err = float(np.abs(d[name].astype(np.float64).reshape(want.shape) - want).max())
            print(f"DET detect {name} photo {k}: e_ref={eref:.3e} e_hip={err:.3e} ratio={err / (eref * sc):.2f} tol={tol:.3e} scale={sc:.4f}")
            assert err <= tol
    # the same photos as one packed device buffer: equal bytes
    flat = torch.from_numpy(np.concatenate([p.reshape(-1) for p in case["photos"]])).to(DEV)
    res2 = detector.detect(device_photos=(flat, [0, case["photos"][0].size], [p.shape[:2] for p in case["photos"]]), side=K.SIDE,
                           threshold=K.THRESHOLD, nms=K.NMS)
    for a, b in zip(res, res2):
        for key in ("landmarks", "box", "score", "prior"):
            assert a[key].tobytes() == b[key].tobytes(), key
    # min_face and max_faces act on the same list
    few = detector.detect(photos=case["photos"], side=K.SIDE, threshold=K.THRESHOLD, nms=K.NMS, max_faces=2)
    assert all(list(f["prior"]) == list(d["prior"][:2]) and f["status"] == R.FACES_CAPPED for f, d in zip(few, res))
    big = detector.detect(photos=case["photos"], side=K.SIDE, threshold=K.THRESHOLD, nms=K.NMS, min_face=40.0)
    for f, d in zip(big, res):
        sel = np.minimum(d["box"][:, 2] - d["box"][:, 0], d["box"][:, 3] - d["box"][:, 1]).astype(np.float64) >= 40.0
        assert list(f["prior"]) == list(d["prior"][sel])
