"""GPU checks of the opt-in device ingest of the loaders: imageio.DeviceRestoreLoader equals RestoreTestSet item by item,
trainset.DegradeLoader(resize="device") equals resize="host", and `restoration_metrics --ingest device` writes the directory
`--ingest host` writes -- all bitwise."""
import os
import random

import numpy as np
import pytest
import torch

from test_metrics_cli_gpu import cli_run  # noqa: F401  (the synthetic checkpoints, images and host-ingest runs of the metrics CLI test)

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMAGES = os.path.join(ROOT, "tests", "golden", "loader_images")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize("im_size", [(64, 64), (48, 80)], ids=["64", "48x80"])
@pytest.mark.parametrize("with_gt", [False, True], ids=["no_gt", "gt"])
def test_device_restore_loader_equals_the_dataset(im_size, with_gt):
    """PNG and JPEG files, a sub-folder, wide, tall and exact-size images; batch sizes 1 and 3 (a ragged last batch); a lo..hi shard"""
    from vspbfr_amd.imageio import DeviceRestoreLoader, RestoreTestSet
    lq_root = os.path.join(IMAGES, "lq")
    hq_root = os.path.join(IMAGES, "hq")
    if with_gt:   # pair the HQ files with LQ files of other sizes too: the HQ's size decides, the LQ is scaled non-uniformly
        data = RestoreTestSet(lq_root, hq_root, im_size)
        assert len(data.lq) == len(data.hq) == 4
    else:
        data = RestoreTestSet(lq_root, None, im_size)
        assert len(data) == 4 and any(p.endswith(".jpg") for p in data.lq) and any(os.sep + "sub" + os.sep in p for p in data.lq)
    want = [data[i] for i in range(len(data))]
    for batch, lo, hi in ((1, 0, 4), (3, 0, 4), (3, 1, 4), (2, 1, 2)):
        seen = []
        for idx, low, gts in DeviceRestoreLoader(data, batch, DEV, lo, hi, threads=2):
            assert low.is_cuda and low.dtype == torch.float32 and tuple(low.shape) == (len(idx), 3) + im_size and len(idx) <= batch
            assert (gts is None) == (not with_gt)
            for k, i in enumerate(idx):
                w = want[i]
                assert torch.equal(_bits(low[k]), _bits(w[0] if with_gt else w)), (batch, i)
                if with_gt:
                    assert torch.equal(_bits(gts[k]), _bits(w[1])), (batch, i)
            seen += idx
        assert seen == list(range(lo, hi))
    assert list(DeviceRestoreLoader(data, 2, DEV, 2, 2)) == []


def test_device_restore_loader_exact_size_pair_mismatch_is_refused(tmp_path):
    """load_pair keeps both images as they are when the HQ has the target size: an LQ of another size cannot be stacked"""
    from PIL import Image
    from vspbfr_amd.imageio import DeviceRestoreLoader, RestoreTestSet
    (tmp_path / "lq").mkdir()
    (tmp_path / "hq").mkdir()
    Image.fromarray(np.zeros((20, 30, 3), np.uint8)).save(tmp_path / "lq" / "a.png")
    Image.fromarray(np.zeros((16, 24, 3), np.uint8)).save(tmp_path / "hq" / "a.png")
    data = RestoreTestSet(str(tmp_path / "lq"), str(tmp_path / "hq"), (16, 24))
    with pytest.raises(ValueError, match="ground truth of the target size"):
        list(DeviceRestoreLoader(data, 1, DEV))


@pytest.mark.parametrize("cls", ["ImageFolder_restore_free_form", "ImageFolder_restore"])
def test_degrade_loader_device_resize_equals_host(cls):
    """two epochs over the four HQ images at 64^2 (flips and random crops occur; the keyed draws make the chain deterministic)"""
    from vspbfr_amd import trainset as T
    ds = getattr(T, cls)(os.path.join(IMAGES, "hq"), im_size=(64, 64))
    host = T.DegradeLoader(ds, 2, device=DEV, seed=11, resize="host")
    dev = T.DegradeLoader(ds, 2, device=DEV, seed=11, resize="device")
    flips = crops = 0
    for epoch in range(2):
        for i in host.indices(epoch):
            _, _, rng = ds.draws(epoch, int(i), 11)
            _, flip, (nw, nh), (x0, y0) = ds.load_raw(int(i), rng)
            flips += flip
            crops += (x0, y0) != (0, 0)
        a, b = list(host.epoch(epoch)), list(dev.epoch(epoch))
        assert len(a) == len(b) == 2
        for ta, tb in zip(a, b):
            assert len(ta) == len(tb) == (3 if ds.n_lq == 2 else 2)
            for x, y in zip(ta, tb):
                assert x.dtype == y.dtype and x.shape == y.shape
                assert torch.equal(x, y) if x.dtype == torch.uint8 else torch.equal(_bits(x), _bits(y))
    assert crops > 0 and (flips > 0 or not ds.flip)
    with pytest.raises(ValueError, match="resize"):
        T.DegradeLoader(ds, 2, device=DEV, resize="gpu")


def test_metrics_cli_device_ingest_writes_the_same_directory(cli_run):  # noqa: F811
    """`--ingest device` against the `--ingest host` (default) runs of the metrics CLI test, from the same seeds and checkpoints: the
    PNGs, and with --metrics the metrics_0.json, byte for byte"""
    from vspbfr_amd import restoration_metrics
    tmp = cli_run["plain"].parents[3]
    ck, lq, hq = tmp / "ckpt", tmp / "lq", tmp / "hq"
    torch.manual_seed(123)
    random.seed(123)
    out = tmp / "eval_device"
    restoration_metrics.main(["--batch", "2", "--ckpt", str(ck / "restoration_net.pt"), "--ddpm_ckpt", str(ck / "code_diffuser.pt"),
                              "--psp_checkpoint_path", str(ck / "style_encoder_decoder.pt"), "--eval_dir", str(out), "--timesteps", "4",
                              "--no_sample", "--lq_data_list", str(lq), "--hq_data_list", str(hq), "--data_name_list", "demo",
                              "--metrics", "--ingest", "device"])
    got, want = out / "restoration_net" / "0" / "demo", cli_run["metrics"]
    names = sorted(os.listdir(want))
    assert sorted(os.listdir(got)) == names and "metrics_0.json" in names and len(names) == 10
    for n in names:
        assert (got / n).read_bytes() == (want / n).read_bytes(), n
    for n in sorted(os.listdir(cli_run["plain"])):
        assert (got / n).read_bytes() == (cli_run["plain"] / n).read_bytes(), n
