"""CPU: the landmark network's host side (vspbfr_amd/fan.py) against the restatement of tests/fan_ref.py -- key layout, loader
rules, BatchNorm reduction, weight image, the entries' refusals (nothing is launched: no GPU), the chunking guard, the NumPy decode,
the CLIs' argument rules and the Evaluator's refusals."""
import json

import numpy as np
import pytest
import torch

import fan_ref as R

NM, DP = 2, 2        # the narrow-depth network of the tests: full channel widths


@pytest.fixture(scope="module")
def small():
    net = R.make_model(0, NM, DP)
    return net, R.state_of(net)


# --------------------------------------------------------------------------------------------------------------------------- layout
def test_key_layout_and_counts_against_the_tree(small):
    from vspbfr_amd import fan
    assert len(fan.expected_state()) == 945 and len(fan.expected_state(with_tracked=True)) == 1129
    assert len(fan.expected_state(NM, DP)) == 321 and len(fan.expected_state(NM, DP, True)) == 383
    for nm, dp, net in ((4, 4, R.FAN(4, 4)), (NM, DP, small[0])):
        tree = {k: tuple(v.shape) for k, v in net.state_dict().items()}
        assert fan.expected_state(nm, dp, with_tracked=True) == tree
        assert list(fan.expected_state(nm, dp, with_tracked=True)) == list(tree)          # the checkpoint's order too
    net4 = R.FAN(4, 4)
    convs = [m for m in net4.modules() if isinstance(m, torch.nn.Conv2d)]
    assert len(convs) == 194 and round(sum(p.numel() for p in net4.parameters()) / 1e5) == 238


def test_loader_rules(small):
    from vspbfr_amd import fan
    _, sd = small
    chk, nm, dp = fan.check_state_dict(sd)
    assert (nm, dp) == (NM, DP) and len(chk) == 321 and all(v.dtype == torch.float64 for v in chk.values())
    assert fan.modules_of(R.state_of(R.FAN(4, 4))) == (4, 4)
    wrapped = {"state_dict": {"module." + k: v for k, v in R.state_of(small[0], tracked=True).items()}}
    chk2, nm2, dp2 = fan.check_state_dict(wrapped)                       # `module.` stripped, counters ignored, the wrapper opened
    assert (nm2, dp2) == (NM, DP) and all(torch.equal(chk[k], chk2[k]) for k in chk)
    miss = {k: v for k, v in sd.items() if k != "m1.b2_plus_1.bn2.running_var"}
    with pytest.raises(ValueError, match=r"missing keys m1\.b2_plus_1\.bn2\.running_var"):
        fan.check_state_dict(miss)
    with pytest.raises(ValueError, match=r"unexpected keys conv5\.weight"):
        fan.check_state_dict(dict(sd, **{"conv5.weight": torch.zeros(1)}))
    with pytest.raises(ValueError, match=r"al0\.weight has shape \(256, 68\), expected \(256, 68, 1, 1\)"):
        fan.check_state_dict(dict(sd, **{"al0.weight": sd["al0.weight"].reshape(256, 68)}))
    with pytest.raises(ValueError, match=r"unexpected keys bl1\.bias"):      # the last module has no bl / al
        fan.check_state_dict(dict(sd, **{"bl1.bias": torch.zeros(256)}))
    with pytest.raises(ValueError, match="missing keys"):                    # three modules asked of a file with two
        fan.check_state_dict(sd, num_modules=3)
    with pytest.raises(ValueError, match="no hourglass module"):
        fan.check_state_dict({"conv1.weight": torch.zeros(64, 3, 7, 7)})
    with pytest.raises(ValueError, match="expected a state dict"):
        fan.check_state_dict([1, 2])
    with pytest.raises(ValueError, match="no such file"):
        fan.check_state_dict("/nonexistent/fan.pth")


def test_torchscript_archive_is_refused(tmp_path, small):
    from vspbfr_amd import fan

    class Tiny(torch.nn.Module):
        def forward(self, x):
            return x + 1

    path = str(tmp_path / "2DFAN4.zip")
    torch.jit.save(torch.jit.script(Tiny()), path)
    assert fan.is_torchscript_archive(path)
    with pytest.raises(ValueError, match="TorchScript archive"):
        fan.FanLandmarks(path, "cpu")
    with pytest.raises(ValueError, match="TorchScript archive"):
        fan.check_state_dict(torch.jit.script(Tiny()))
    good = str(tmp_path / "fan.pth")
    torch.save(small[1], good)                                              # a state dict in torch's zip format is none
    assert not fan.is_torchscript_archive(good)
    assert fan.check_state_dict(good)[1:] == (NM, DP)


# ------------------------------------------------------------------------------------------------------------------------ reduction
def _as_ref(red):
    """the product's reduced state under the restatement's shapes: `al` without its zero padding"""
    return {k: (v[:, :R.POINTS] if k.startswith("al") and k.endswith(".w") else v) for k, v in red.items()}


def test_reduction_against_the_unfused_tree(small):
    from vspbfr_amd import fan
    net, sd = small
    chk, nm, dp = fan.check_state_dict(sd)
    red = fan.reduce_state(chk, nm, dp)
    assert set(_as_ref(red)) == set(R.reduce(sd, nm, dp))
    assert all(v.dtype == torch.float64 for v in red.values())
    assert tuple(red["al0.w"].shape) == (256, fan.POINTS_PAD, 1, 1) and not red["al0.w"][:, R.POINTS:].any()
    # a whole-image box at the image's own side samples every pixel exactly: the crop is photo / 255
    photos = np.stack([R.test_photo(48, 48, 1), R.test_photo(48, 48, 2)])
    boxes = np.array([[0, 0, 48], [0, 0, 48]], np.float32)
    x = torch.as_tensor(photos).permute(0, 3, 1, 2).double() / 255
    assert torch.equal(R.crop_ref(photos, boxes, 48, torch.float64), x)
    with torch.no_grad():
        want = net(x)
    got = R.forward(_as_ref(red), photos, boxes, 48, nm, dp, torch.float64, rounded=False)
    rel = float((got - want).abs().max() / want.abs().max())
    print(f"FAN reduction vs the unfused tree: {rel:.3e} relative")
    assert rel <= 1e-12
    # for a 2 s x 2 s face and side s the crop is the exact 2 x 2 mean
    big = np.stack([R.test_photo(32, 32, 3)])
    mean = torch.nn.functional.avg_pool2d(torch.as_tensor(big).permute(0, 3, 1, 2).double(), 2) / 255
    assert torch.equal(R.crop_ref(big, np.array([[0, 0, 32]], np.float32), 16, torch.float64), mean)


def test_float64_stream_stays_far_from_the_f16_range(small):
    from vspbfr_amd import fan
    photos = np.stack([R.test_photo(80, 80, 1), R.test_photo(80, 80, 2)])
    boxes = np.array([[0, 0, 80], [5.5, -3, 70]], np.float32)
    for seed in range(3):
        sd = R.state_of(R.make_model(seed, NM, DP))
        watch = []
        R.forward(R.reduce(sd, NM, DP), photos, boxes, 64, NM, DP, torch.float64, watch=watch)
        print(f"FAN seed {seed}: the float64 stream peaks at {max(watch):.1f}")
        assert max(watch) < 1e3


def test_weight_image_by_index_and_round_trip(small):
    from vspbfr_amd import fan
    g = torch.Generator().manual_seed(3)
    for co, ci, k in ((68, 256, 1), (256, 96, 1), (32, 64, 3), (128, 256, 3)):
        w = torch.randn(co, ci, k, k, generator=g, dtype=torch.float64).float().half()
        img = fan.pack_conv_weight(w)
        cp = (co + 31) // 32 * 32
        assert tuple(img.shape) == (k * k, ci // 32, cp // 16, 64, 8)
        assert torch.equal(fan.unpack_conv_weight(img, co), w) and not fan.unpack_conv_weight(img)[co:].any()
        flat = img.reshape(-1)
        for a, b, t in ((0, 0, 0), (co - 1, ci - 1, k * k - 1), (17, 41, (k * k) // 2), (co // 2 + 3, 9, 0)):
            assert flat[R.pack_index(a, b, t, ci, co)] == w[a, b, t // k, t % k]
    with pytest.raises(ValueError, match="pack_conv_weight"):
        fan.pack_conv_weight(torch.zeros(32, 68, 1, 1))
    net = fan.FanLandmarks(small[1], "cpu", side=64)
    assert net.image.dtype == torch.float16 and len(net.index) == len([k for k in net.reduced if k.endswith(".w")]) - 1
    d = net.describe()
    assert (d["num_modules"], d["depth"], d["side"], d["points"], d["convolutions"]) == (NM, DP, 64, 68, len(net.index) + 1)
    for name in ("conv2.conv1", "m1.b2_plus_1.conv3", "l1", "al0", "conv_last0"):
        at, shape, cout = net.index[name]
        w = net.reduced[name + ".w"]
        assert at % 8 == 0 and cout == w.shape[0]
        img, _ = net._w(name)
        assert torch.equal(fan.unpack_conv_weight(img, cout), w.float().half())      # rounded once, from float64 through fp32
        co, ci, t = cout - 1, w.shape[1] // 2 + 1, shape[0] - 1
        k = w.shape[2]
        assert net.image[at + R.pack_index(co, ci, t, w.shape[1], cout)] == w[co, ci, t // k, t % k].float().half()
    assert all(v.dtype == torch.float32 for v in net.p.values()) and tuple(net.p["conv1.w"].shape) == (147, 64)
    assert torch.equal(net.p["conv1.w"][(7 * 2 + 5) * 3 + 1], net.reduced["conv1.w"][:, 1, 2, 5].float())
    with pytest.raises(ValueError, match="side 40"):
        fan.FanLandmarks(small[1], "cpu", side=40)


# ------------------------------------------------------------------------------------------------------------------------- refusals
P = 4096      # a non-null, 16-byte aligned dummy address: never dereferenced on these paths


def _conv(**kw):
    from vspbfr_amd import _lib
    a = dict(y=P, y_pitch=256, y_off=0, raw=None, raw_pitch=0, raw_off=0, x=2 * P + (1 << 24), x_pitch=256, x_off=0, B=2, H=8, W=8, Cin=256, Cout=128,
             ksize=3, flags=0, w=3 * P + (2 << 24), b=None, ia=None, ib=None, res1=None, res1_pitch=0, res1_off=0, res2=None, res2_pitch=0,
             res2_off=0, up=None, up_pitch=0, up_off=0)
    assert set(kw) <= set(a), set(kw) - set(a)
    a.update(kw)
    rc = _lib.lib.vsp_fan_conv_f16(*a.values(), None)
    return rc, _lib.last_error()


FAR = 5 * P + (8 << 24)


@pytest.mark.parametrize("kw,msg", [
    (dict(Cin=68), "68 input channels"), (dict(Cin=288), "288 input channels"), (dict(Cin=16), "16 input channels"),
    (dict(Cout=48), "48 output channels"), (dict(Cout=288), "288 output channels"), (dict(Cout=64 + 4), None),
    (dict(ksize=5), "filter 5 x 5"), (dict(flags=4), "unknown flags"),
    (dict(x_off=8), "input channels 8..263 of a pitch of 256"), (dict(x_pitch=260), "input channels"), (dict(x_off=-8), "input channels"),
    (dict(y_off=192), "output channels 192..319"), (dict(y_pitch=130), "output channels"),
    (dict(raw=FAR, raw_pitch=64, raw_off=0), "raw channels 0..127 of a pitch of 64"),
    (dict(res1=FAR, res1_pitch=128, res1_off=2), "residual channels"),
    (dict(res1=FAR, res1_pitch=128, res2=FAR + (4 << 24), res2_pitch=64), "second residual channels"),
    (dict(res2=FAR, res2_pitch=128), "a second residual without a first"),
    (dict(up=FAR, up_pitch=100), "coarser-level channels"),
    (dict(ia=FAR), "needs both a and b"),
    (dict(y=None), "null pointer"), (dict(w=None), "null pointer"),
    (dict(x=2 * P + (1 << 24) + 8), "aligned"), (dict(y=P + 4), "aligned"), (dict(flags=2, y=P + 8), "aligned"), (dict(b=FAR + 4), "aligned"),
    (dict(up=FAR, up_pitch=128, H=7), "even map, not 7 x 8"),
    (dict(x=P + 64), "an output overlaps the input"),
    (dict(raw=2 * P + (1 << 24), raw_pitch=128), "an output overlaps the input"),
    (dict(raw=P, raw_pitch=128), "the raw output overlaps the output"),
    (dict(res1=P + 8, res1_pitch=256), "a residual overlaps the output without being its window"),
    (dict(res1=P, res1_pitch=256, res1_off=128), "a residual overlaps the output without being its window"),
    (dict(res1=P, res1_pitch=256, flags=2), "a residual overlaps the output without being its window"),
    (dict(raw=FAR, raw_pitch=128, res1=FAR, res1_pitch=128), "a residual overlaps the raw output"),
    (dict(up=P, up_pitch=256), "the coarser level overlaps an output"),
    (dict(B=-1), "batch -1"), (dict(H=0), "map 0 x 8"), (dict(W=5000), "map 8 x 5000"),
])
def test_conv_entry_refusals(kw, msg):
    from vspbfr_amd import _lib
    rc, err = _conv(**kw)
    if msg is None:          # 68 output channels are served: this call passes the validation and would launch, so only its B = 0 form is made
        assert _conv(B=0, **kw)[0] == 0
        return
    assert rc == -1 and msg in err, (rc, err)
    assert _lib.lib.vsp_fan_conv_f16 is not None


def test_conv_entry_accepts_what_it_serves_without_launching():
    """B = 0 returns VSP_OK behind the shape checks and before the pointer checks; 2 GiB is VSP_ENOTSUP; the in-place window is legal"""
    assert _conv(B=0)[0] == 0 and _conv(B=0, y=None, x=None, w=None)[0] == 0
    assert _conv(B=0, Cin=48)[0] == -1
    rc, err = _conv(B=4, H=4096, W=4096, Cin=32, Cout=32, x_pitch=32, y_pitch=32)
    assert rc == -3 and "2 GiB" in err
    rc, err = _conv(B=2, H=2048, W=2048, Cin=32, Cout=68, x_pitch=32, y_pitch=68, flags=2, y=FAR)       # fp32: 4 bytes a value
    assert rc == -3 and "2 GiB" in err


def test_stem_pool_decode_entry_refusals():
    from vspbfr_amd import _lib
    L, err = _lib.lib, _lib.last_error
    stem = lambda **k: L.vsp_fan_stem_u8(*dict(dict(y=P, src=FAR, box=2 * P, w=3 * P, b=4 * P, B=2, H=37, W=53, side=32), **k).values(), None)
    for kw, msg in ((dict(side=36), "side 36"), (dict(side=4), "side 4"), (dict(side=2048), "side 2048"), (dict(H=0), "photo 0 x 53"),
                    (dict(B=70000), "batch 70000"), (dict(box=None), "null pointer"), (dict(y=P + 4), "aligned"), (dict(w=3 * P + 4), "aligned")):
        assert stem(**kw) == -1 and msg in err(), (kw, err())
    assert stem(B=0) == 0 and stem(B=0, y=None) == 0
    assert stem(B=60, H=4096, W=4096) == -3 and "2 GiB" in err()
    pool = lambda **k: L.vsp_fan_pool_f16(*dict(dict(y=P, y_pitch=128, y_off=0, x=FAR, x_pitch=128, x_off=0, B=2, H=8, W=10, C=128), **k).values(), None)
    for kw, msg in ((dict(H=7), "an odd map, 7 x 10"), (dict(W=5), "an odd map"), (dict(C=260), "260 channels"), (dict(C=12), "12 channels"),
                    (dict(x_off=4), "input channels"), (dict(y_pitch=64), "output channels 0..127 of a pitch of 64"), (dict(x=None), "null pointer"),
                    (dict(y=P + 8), "16-byte aligned"), (dict(x=P + 64), "the output overlaps the input")):
        assert pool(**kw) == -1 and msg in err(), (kw, err())
    assert pool(B=0) == 0
    assert pool(B=64, H=4096, W=4096, C=8, x_pitch=8, y_pitch=8) == -3
    dec = lambda **k: L.vsp_fan_decode_f32(*dict(dict(lm=P, peak=2 * P, flag=3 * P, hm=FAR, pitch=68, box=4 * P, B=2, n=16, K=68), **k).values(), None)
    for kw, msg in ((dict(n=0), "map 0 x 0"), (dict(n=2000), "map 2000"), (dict(K=0), "0 landmarks"), (dict(pitch=64), "68 landmarks in a pitch of 64"),
                    (dict(flag=None), "null pointer"), (dict(hm=FAR + 2), "4-byte aligned"), (dict(B=-2), "batch -2")):
        assert dec(**kw) == -1 and msg in err(), (kw, err())
    assert dec(B=0) == 0
    assert dec(B=2000, n=1024, pitch=68) == -3


# ------------------------------------------------------------------------------------------------------------------------ the guard
def test_the_guard_runs_a_large_group_in_chunks_of_images(small, monkeypatch):
    from vspbfr_amd import fan
    net = fan.FanLandmarks(small[1], "cpu", side=64)
    assert fan.image_bytes(256) == 128 * 128 * 128 * 2 and (fan.FanLandmarks.GUARD_BYTES - 1) // fan.image_bytes(256) == 511
    seen = []

    def fake(u8, box):
        seen.append((int(u8.shape[0]), box.clone()))
        return (u8[:, 0, 0, 0].float().view(-1, 1).expand(-1, 16 * 16 * 68) + box[:, :1]).contiguous().view(-1)

    monkeypatch.setattr(net, "_network", fake)
    u8 = torch.arange(5, dtype=torch.uint8).view(5, 1, 1, 1).expand(5, 70, 70, 3).contiguous()
    boxes = torch.tensor([[100.0 * i, 0, 70] for i in range(5)])
    whole = net.heatmaps(u8, boxes)
    assert [s[0] for s in seen] == [5] and tuple(whole.shape) == (5, 68, 16, 16)
    seen.clear()
    monkeypatch.setattr(net, "GUARD_BYTES", 2 * fan.image_bytes(64) + 1)
    split = net.heatmaps(u8, boxes)
    assert [s[0] for s in seen] == [2, 2, 1] and torch.equal(seen[2][1], boxes[4:]) and torch.equal(split, whole)
    monkeypatch.setattr(net, "GUARD_BYTES", fan.image_bytes(64))
    with pytest.raises(ValueError, match="not served"):
        net.heatmaps(u8, boxes)
    monkeypatch.setattr(net, "GUARD_BYTES", 1 << 31)
    assert tuple(net.heatmaps(u8[:0], boxes[:0]).shape) == (0, 68, 16, 16)
    # the photos of a chunk count like its activations: 400 x 400 x 3 bytes an image are more than the 131 072 of conv2's output
    big = torch.arange(5, dtype=torch.uint8).view(5, 1, 1, 1).expand(5, 400, 400, 3).contiguous()
    monkeypatch.setattr(net, "GUARD_BYTES", 2 * 400 * 400 * 3 + 1)
    seen.clear()
    assert torch.equal(net.heatmaps(big, boxes), whole) and [s[0] for s in seen] == [2, 2, 1]
    monkeypatch.setattr(net, "GUARD_BYTES", 400 * 400 * 3)
    with pytest.raises(ValueError, match="a photo or an activation tensor of 480000 bytes"):
        net.heatmaps(big, boxes)
    monkeypatch.setattr(net, "GUARD_BYTES", 1 << 31)
    # one box for every image is filled in where the network runs; per-image boxes may come as a list
    assert net.boxes(u8, [[1, 2, 3]] * 5).tolist() == [[1.0, 2.0, 3.0]] * 5
    # boxes: the default is the whole image, one triple serves every image, a wrong shape is refused
    assert net.boxes(u8).tolist() == [[0.0, 0.0, 70.0]] * 5 and net.boxes(u8, (1, 2, 30)).tolist() == [[1.0, 2.0, 30.0]] * 5
    with pytest.raises(ValueError, match="boxes"):
        net.boxes(u8, torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="uint8"):
        net.heatmaps(u8.float())


# --------------------------------------------------------------------------------------------------------------------- NumPy decode
def test_numpy_decode_cases():
    n = 8
    heat = np.zeros((1, 6, n, n), np.float32)
    box = np.array([[10.0, 20.0, 64.0]], np.float32)       # 8 image pixels per heatmap cell
    heat[0, 0, 3, 5] = heat[0, 0, 6, 2] = 2.0               # a tie: the lowest flat index; neighbours equal: no offset
    heat[0, 1, 0, 4] = 3.0                                  # a border peak in y: no offset there, one in x
    heat[0, 1, 0, 5], heat[0, 1, 0, 3] = 1.0, 0.5
    heat[0, 2, 4, 4], heat[0, 2, 4, 3], heat[0, 2, 4, 5] = 5.0, 1.0, 1.0    # a zero difference in x
    heat[0, 2, 3, 4], heat[0, 2, 5, 4] = 2.0, 1.0                           # and a negative one in y
    heat[0, 3, 7, 7] = 1.0                                  # the last corner
    heat[0, 4] = -1.0                                       # a constant map: index 0
    heat[0, 5, 2, 2], heat[0, 5, 1, 1] = np.nan, 4.0        # a NaN never wins and is flagged
    lm, peak, bad = R.decode_ref(heat, box)
    want = [(10 + 5.5 * 8, 20 + 3.5 * 8), (10 + 4.75 * 8, 20 + 0.5 * 8), (10 + 4.5 * 8, 20 + 4.25 * 8), (10 + 7.5 * 8, 20 + 7.5 * 8),
            (10 + 0.5 * 8, 20 + 0.5 * 8), (10 + 1.5 * 8, 20 + 1.5 * 8)]
    assert lm[0].tolist() == [list(w) for w in want]
    assert peak[0].tolist() == [2.0, 3.0, 5.0, 1.0, -1.0, 4.0] and bad.tolist() == [True]
    assert R.decode_ref(heat[:, :5], box)[2].tolist() == [False]
    heat[0, 5] = np.inf
    lm, peak, bad = R.decode_ref(heat, box)
    assert lm[0, 5].tolist() == [14.0, 24.0] and peak[0, 5] == -np.inf and bad.tolist() == [True]
    d, e = R.lmd_nme_ref(np.zeros((1, 68, 2)) + [[3.0, 4.0]], np.zeros((1, 68, 2)) + np.arange(68).reshape(68, 1) * [0.0, 0.0])
    assert d.tolist() == [5.0] and np.isinf(e[0])
    g = np.zeros((1, 68, 2))
    g[0, 45] = [10.0, 0.0]
    a = g + [[0.0, 2.0]]
    d, e = R.lmd_nme_ref(a, g)
    assert d.tolist() == [2.0] and e.tolist() == [0.2]


# -------------------------------------------------------------------------------------------------------------------------- the CLIs
@pytest.mark.parametrize("argv,msg", [
    (["--restored", "d", "--gt", "g", "--lmd_box", "0,0,512"], "--lmd_box only has a meaning with --lmd_weights"),
    (["--restored", "d", "--niqe_params", "p.npz", "--lmd_weights", "w.pth"], "--lmd_weights measures against ground truth"),
    (["--restored", "d", "--gt", "g", "--lmd_weights", "/nonexistent/w.pth"], "no such file"),
    (["--restored", "d", "--gt", "g", "--lmd_weights", __file__, "--lmd_box", "0,0"], "a box is X0,Y0,SIDE"),
    (["--restored", "d", "--gt", "g", "--lmd_weights", __file__, "--lmd_box", "0,0,-4"], "positive side"),
])
def test_score_argument_rules(argv, msg, capsys):
    from vspbfr_amd import score
    with pytest.raises(SystemExit) as e:
        score.main(argv)
    assert e.value.code == 2 and msg in capsys.readouterr().err


@pytest.mark.parametrize("argv,msg", [
    (["--lmd_weights", "w.pth", "--lq_data_list", "a", "--hq_data_list", "b", "--data_name_list", "n"], "--lmd_weights only has a meaning with --metrics"),
    (["--metrics", "--lmd_weights", "w.pth", "--lq_data_list", "a,c", "--hq_data_list", "b,None", "--data_name_list", "n,m"],
     "--lmd_weights measures against ground truth"),
    (["--metrics", "--lmd_box", "0,0,512", "--lq_data_list", "a", "--hq_data_list", "b", "--data_name_list", "n"],
     "--lmd_box only has a meaning with --lmd_weights"),
])
def test_restoration_metrics_argument_rules(argv, msg, capsys):
    from vspbfr_amd import restoration_metrics
    with pytest.raises(SystemExit) as e:
        restoration_metrics.main(argv)
    assert e.value.code == 2 and msg in capsys.readouterr().err


def test_help_texts_name_the_flags(capsys):
    from vspbfr_amd import fan, restoration_metrics, score
    for main, words in ((score.main, ("--lmd_weights", "--lmd_box", "2D-FAN")), (restoration_metrics.main, ("--lmd_weights", "--lmd_box")),
                        (fan.main, ("--faces", "--weights", "--out", "--box", "68"))):
        with pytest.raises(SystemExit) as e:
            main(["--help"])
        out = capsys.readouterr().out
        assert e.value.code == 0 and all(w in out for w in words), out
    with pytest.raises(SystemExit) as e:
        fan.main(["--faces", "d", "--weights", "w", "--out", "o", "--box", "1,2"])
    assert e.value.code == 2 and "a box is X0,Y0,SIDE" in capsys.readouterr().err
    assert fan.parse_box("1.5,-2,300") == (1.5, -2.0, 300.0)
    txt = fan.landmarks68_json({"a.png": np.array([[0.1, 2.5]] * 68, np.float32)})
    back = json.loads(txt)
    assert list(back) == ["a.png"] and len(back["a.png"]) == 68 and np.float32(back["a.png"][0][0]) == np.float32(0.1)


# --------------------------------------------------------------------------------------------------------------------- the Evaluator
ROWS = [{"index": 1, "lq": "b", "hq": "b", "sse": 12, "psnr": 40.5, "ssim": 0.9, "lpips": 0.25},
        {"index": 0, "lq": "a", "hq": "a", "sse": 0, "psnr": None, "ssim": 1.0, "lpips": 0.0}]


def test_evaluator_refusals_and_a_report_without_lmd_is_the_parents(tmp_path):
    from vspbfr_amd import metrics as M
    with pytest.raises(ValueError, match="lmd_box only has a meaning with lmd"):
        M.Evaluator(lmd_box=(0, 0, 512))
    ev = M.Evaluator(niqe=(np.zeros(36), np.eye(36)), lmd=object())
    with pytest.raises(RuntimeError, match="NIQE only"):
        ev.add(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), None)
    # without the columns, the summary, its line and a merge are what they were: no key, no word about lmd
    rep = M.summarize([dict(r) for r in ROWS], "d", "gauss11")
    assert rep == {"dataset": "d", "count": 2, "window": "gauss11", "psnr_infinite": 1, "mean": {"psnr": 40.5, "ssim": 0.95, "lpips": 0.125},
                   "images": [ROWS[1], ROWS[0]]}
    assert list(rep["mean"]) == ["psnr", "ssim", "lpips"]
    assert M.summary_line(rep) == "metrics d (gauss11, 2 images, 1 identical): psnr 40.5, ssim 0.95, lpips 0.125"
    assert M.Evaluator().report("d") == {"dataset": "d", "count": 0, "window": "gauss11", "psnr_infinite": 0, "mean": {}, "images": []}
    # with them, the means are carried like lpips' (None left out) through summary, line and merge
    with_lmd = [dict(ROWS[0], lmd=2.0, nme=0.02), dict(ROWS[1], lmd=None, nme=None)]
    rep = M.summarize(with_lmd, "d", "gauss11")
    assert rep["mean"]["lmd"] == 2.0 and rep["mean"]["nme"] == 0.02 and list(rep["mean"]) == ["psnr", "ssim", "lpips", "lmd", "nme"]
    assert M.summary_line(rep).endswith("lpips 0.125, lmd 2, nme 0.02")
    paths = []
    for k, row in enumerate(([dict(ROWS[0], lmd=2.0, nme=0.02)], [dict(ROWS[1], lmd=4.0, nme=0.06)])):
        paths.append(str(tmp_path / f"metrics_{k}.json"))
        M.write_report(M.summarize(row, "d", "gauss11"), paths[-1])
    merged = M.merge_reports(paths)
    assert merged["mean"]["lmd"] == 3.0 and merged["mean"]["nme"] == pytest.approx(0.04) and merged["count"] == 2
