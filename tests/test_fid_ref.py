"""CPU checks of the FID restatement (tests/fid_ref.py) and of the loader and fold of vspbfr_amd/fid.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fid_ref as R


def test_key_set_is_94_times_5_plus_the_ignored():
    from vspbfr_amd import fid
    want = fid.expected_state()
    assert len(fid.convs()) == 94 and len(want) == 94 * 5
    sd = R.shared_state()
    tracked = [k for k in sd if k.endswith("num_batches_tracked")]
    assert len(tracked) == 94 and set(sd) - set(tracked) == set(want)
    for k, shape in want.items():
        assert tuple(sd[k].shape) == tuple(shape), k
    assert want["Mixed_6b.branch7x7dbl_3.conv.weight"] == (128, 128, 1, 7)
    assert want["Mixed_7c.branch3x3dbl_2.conv.weight"] == (384, 448, 3, 3)
    assert want["Conv2d_1a_3x3.conv.weight"] == (32, 3, 3, 3)


def test_loader_strips_ignores_and_refuses_by_name():
    from vspbfr_amd import fid
    sd = dict(R.shared_state())
    st = fid.check_state_dict(sd)
    assert len(st.tensors) == 470 and fid.check_state_dict(st) is st
    # module. is stripped; fc.*, AuxLogits.* and num_batches_tracked are ignored, present or not
    wrapped = {"module." + k: v for k, v in sd.items()}
    wrapped.update({"module.fc.weight": torch.zeros(1008, 2048), "fc.bias": torch.zeros(1008), "AuxLogits.conv0.conv.weight": torch.zeros(1)})
    assert set(fid.check_state_dict(wrapped).tensors) == set(st.tensors)
    bare = {k: v for k, v in sd.items() if not k.endswith("num_batches_tracked")}
    assert set(fid.check_state_dict(bare).tensors) == set(st.tensors)
    with pytest.raises(ValueError, match="expected a state dict"):
        fid.check_state_dict([1, 2])
    missing = dict(sd)
    del missing["Mixed_6b.branch7x7dbl_3.bn.running_var"]
    with pytest.raises(ValueError, match=r"missing keys Mixed_6b\.branch7x7dbl_3\.bn\.running_var"):
        fid.check_state_dict(missing)
    extra = dict(sd)
    extra["Mixed_8a.branch1x1.conv.weight"] = torch.zeros(1)
    with pytest.raises(ValueError, match=r"unexpected keys Mixed_8a\.branch1x1\.conv\.weight"):
        fid.check_state_dict(extra)
    extra = dict(sd)
    extra["Conv2d_1a_3x3.conv.bias"] = torch.zeros(32)
    with pytest.raises(ValueError, match=r"unexpected keys Conv2d_1a_3x3\.conv\.bias"):
        fid.check_state_dict(extra)
    shaped = dict(sd)
    shaped["Mixed_7a.branch7x7x3_2.conv.weight"] = torch.zeros(192, 192, 7, 1)
    with pytest.raises(ValueError, match=r"Mixed_7a\.branch7x7x3_2\.conv\.weight has shape \(192, 192, 7, 1\), expected \(192, 192, 1, 7\)"):
        fid.check_state_dict(shaped)
    shaped = dict(sd)
    shaped["Mixed_5b.branch_pool.bn.bias"] = torch.zeros(64)
    with pytest.raises(ValueError, match=r"Mixed_5b\.branch_pool\.bn\.bias has shape"):
        fid.check_state_dict(shaped)


def test_fold_of_the_library_equals_the_restatement_and_the_unfused_tree():
    """Folded against unfused in float64.  A layer's fold perturbs its output by a few float64 eps relative, and summing K products in
    another order by at most K eps; the He-conditioned layers have gain about 1, so over the longest path (depth 47 with the pools) the
    features move by at most depth * Kmax * eps64 * max |feature|: 47 * 4032 * 2.2e-16 * max."""
    from vspbfr_amd import fid
    sd = R.shared_state()
    folded = fid.fold_state(sd)
    tree = R.build(sd, torch.float64, folded=True)
    for name, (w, b) in folded.items():
        m = tree.get_submodule(name)
        assert w.dtype == torch.float64 and torch.equal(w, m.conv.weight.data) and torch.equal(b, m.folded_bias), name
    imgs = R.case_images("n107")
    with torch.no_grad():
        got = tree(imgs, resize=False)
    ref64, _ = R.case_reference("n107")
    lim = 47 * 4032 * np.finfo(np.float64).eps * float(ref64.abs().max())
    err = float((got - ref64).abs().max())
    print(f"fold: err {err:.3g} bound {lim:.3g}")
    assert err <= lim
    # the packed layout of the kernels
    w = folded["Mixed_6b.branch7x7_2"][0]
    p = fid.pack_weight(w)
    assert p.shape == (1, 7, 128, 128) and p.dtype == torch.float32 and float(p[0, 3, 5, 9]) == float(w[9, 5, 0, 3].float())


def test_resize_is_interpolate_bilinear_without_antialias():
    g = torch.Generator().manual_seed(3)
    for h, w in ((512, 512), (64, 97), (75, 75), (299, 299), (1024, 600)):
        x = torch.randint(0, 256, (1, 3, h, w), generator=g).double()
        want = F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False)
        got = R.resize_bilinear(x, 299)
        assert float((got - want).abs().max()) <= 255 * 64 * np.finfo(np.float64).eps * max(h, w)
        if (h, w) == (299, 299):
            assert torch.equal(got, x)
    # down by more than 2: no anti-aliasing, a bilinear sample of four pixels only
    x = torch.zeros(1, 1, 1196, 1196, dtype=torch.float64)
    x[0, 0, ::4, ::4] = 255.0
    assert float(R.resize_bilinear(x, 299).max()) <= 255.0 * 0.25 + 1e-9


def test_pool_rules():
    g = torch.Generator().manual_seed(4)
    for h, w in ((1, 1), (3, 3), (7, 8), (35, 35)):
        x = torch.randn((2, 5, h, w), generator=g, dtype=torch.float64)
        assert float((R.avg_pool_valid(x) - F.avg_pool2d(x, 3, 1, 1, count_include_pad=False)).abs().max()) <= 1e-14
        assert torch.equal(R.max_pool_s1(x), F.max_pool2d(x, 3, 1, 1))
        if h >= 3:
            assert torch.equal(R.max_pool_s2(x), F.max_pool2d(x, 3, 2))
    x = torch.randn((1, 2, 5, 5), generator=g, dtype=torch.float64)
    assert float((R.avg_pool_valid(x) - F.avg_pool2d(x, 3, 1, 1)).abs().max()) > 1e-3          # not count_include_pad=True


def test_mixed_7c_pools_with_max_where_7b_averages():
    tree = R.build(R.shared_state(), torch.float64)
    assert tree.Mixed_7b.pool == "avg" and tree.Mixed_7c.pool == "max"
    from vspbfr_amd import fid
    from vspbfr_amd import hip_ops as H
    pools = [op[1] for op in fid._Plan(299, 299).ops if op[0] == "pool"]
    # two stem pools, 3 A, B, 4 C, D, 7b, 7c, global
    assert pools == [H.FID_POOL_MAX_S2] * 2 + [H.FID_POOL_AVG_S1] * 3 + [H.FID_POOL_MAX_S2] + [H.FID_POOL_AVG_S1] * 4 + [
        H.FID_POOL_MAX_S2, H.FID_POOL_AVG_S1, H.FID_POOL_MAX_S1, H.FID_POOL_GLOBAL_AVG]
    g = torch.Generator().manual_seed(9)
    x = torch.randn((1, 2048, 3, 3), generator=g, dtype=torch.float64)
    with torch.no_grad():
        as_max = tree.Mixed_7c(x)
        tree.Mixed_7c.pool = "avg"
        as_avg = tree.Mixed_7c(x)
    assert torch.equal(as_max[:, :1856], as_avg[:, :1856]) and not torch.equal(as_max[:, 1856:], as_avg[:, 1856:])


def test_output_size_chain():
    from vspbfr_amd import fid
    assert fid.map_chain(299) == [149, 147, 147, 73, 73, 71, 35, 17, 8]
    assert fid.map_chain(75) == [37, 35, 35, 17, 17, 15, 7, 3, 1]
    assert fid.map_chain(107)[-1] == 2
    with pytest.raises(ValueError, match="too small"):
        fid.map_chain(74)
    sizes = []
    with torch.no_grad():
        R.build(R.shared_state(), torch.float32, folded=True)(R.case_images("n75"), resize=False, sizes=sizes)
    chain = [s for i, s in enumerate(sizes) if i < 7 or s != sizes[i - 1]]
    assert chain == [37, 35, 35, 17, 17, 15, 7, 3, 1]
    # the plan writes every channel of every block output exactly once
    plan = fid._Plan(299, 299)
    assert len([op for op in plan.ops if op[0] == "conv"]) == 93
    spans, block = {}, None
    for op in plan.ops:
        if op[0] == "conv" and not op[1].startswith("Mixed"):
            continue
        if op[0] == "conv":
            block = op[1].split(".")[0]
        dst, c = op[3], plan.specs[op[1]].cout if op[0] == "conv" else op[6]
        if block is not None and dst[0] in ("x", "y"):
            assert dst[2] == fid.BLOCK_OUT[block]
            spans.setdefault(block, []).append((dst[1], dst[1] + c))
    assert list(spans) == [b[0] for b in fid.BLOCKS]
    for block, sp in spans.items():
        sp.sort()
        assert sp[0][0] == 0 and sp[-1][1] == fid.BLOCK_OUT[block] and all(a[1] == b[0] for a, b in zip(sp, sp[1:])), (block, sp)


@pytest.mark.parametrize("name", ["n75", "n107", "full"])
def test_features_of_the_gpu_cases_are_alive(name):
    """the float64 features of the very inputs the GPU tests use: a standard deviation between 0.05 and 20, no dead network"""
    ref64, ref32 = R.case_reference(name)
    assert ref64.shape == (R.CASES[name]["n"], 2048) and torch.isfinite(ref64).all()
    assert 0.05 <= float(ref64.std()) <= 20.0
    for row in ref64:
        assert int((row != 0).sum()) > 1024
    e_ref = float((ref32.double() - ref64).abs().max())
    print(f"{name}: std {float(ref64.std()):.3g} max {float(ref64.abs().max()):.3g} e_ref {e_ref:.3g}")
    assert 0 < e_ref < 1e-4
