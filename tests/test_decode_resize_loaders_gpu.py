"""GPU checks of the device decode of the test-time loader: imageio.DeviceRestoreLoader(decode="device") -- baseline JPEG files decoded
on the device and resized where the decoder wrote them, everything else decoded by Pillow -- equals RestoreTestSet item by item, names
the route every file took, and `restoration_metrics --ingest device --decode device` writes the directory `--ingest host` writes.  All
bitwise."""
import os
import random

import pytest
import torch

import resample_ref as R
from test_metrics_cli_gpu import cli_run  # noqa: F401  (the synthetic checkpoints and images of the metrics CLI test)

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMAGES = os.path.join(ROOT, "tests", "golden", "loader_images")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _compare(data, with_gt, im_size, shards, threads=2):
    from vspbfr_amd.imageio import DeviceRestoreLoader
    want = [data[i] for i in range(len(data))]
    how = {}
    for batch, lo, hi in shards:
        seen = []
        loader = DeviceRestoreLoader(data, batch, DEV, lo, hi, threads=threads, decode="device")
        for idx, low, gts in loader:
            assert low.is_cuda and low.dtype == torch.float32 and tuple(low.shape) == (len(idx), 3) + tuple(im_size) and len(idx) <= batch
            assert (gts is None) == (not with_gt)
            for k, i in enumerate(idx):
                w = want[i]
                assert torch.equal(_bits(low[k]), _bits(w[0] if with_gt else w)), (batch, i, data.lq[i])
                if with_gt:
                    assert torch.equal(_bits(gts[k]), _bits(w[1])), (batch, i, data.hq[i])
            seen += idx
        assert seen == list(range(lo, hi))
        how.update(loader.how)
    return how


@pytest.mark.parametrize("im_size", [(64, 64), (48, 80)], ids=["64", "48x80"])
@pytest.mark.parametrize("with_gt", [False, True], ids=["no_gt", "gt"])
def test_device_decode_loader_equals_the_dataset(im_size, with_gt):
    """the committed folder (PNG and JPEG files, a sub-folder, wide, tall and exact-size images): batch sizes 1 and 3, a shard"""
    from vspbfr_amd.imageio import DeviceRestoreLoader, RestoreTestSet
    data = RestoreTestSet(os.path.join(IMAGES, "lq"), os.path.join(IMAGES, "hq") if with_gt else None, im_size)
    assert len(data) == 4 and any(p.endswith(".jpg") for p in data.lq) and any(os.sep + "sub" + os.sep in p for p in data.lq)
    how = _compare(data, with_gt, im_size, ((1, 0, 4), (3, 0, 4), (3, 1, 4), (2, 1, 2)))
    assert set(how) == set(data.lq) | set(data.hq or [])
    assert all(v == "host" for p, v in how.items() if p.endswith(".png")) and set(how.values()) <= {"host", "device"}
    assert list(DeviceRestoreLoader(data, 2, DEV, 2, 2, decode="device")) == []


def _write_set(root, seed):
    """one file of every kind the decoder meets -> {name: the route it must take}"""
    from PIL import Image
    from vspbfr_amd import jpeg
    os.makedirs(root)
    sizes = [(93, 75), (64, 48), (120, 50), (70, 90), (57, 61), (40, 100)]          # (w, h)
    a = [R.test_image(w, h, seed=seed + k) for k, (w, h) in enumerate(sizes)]
    Image.fromarray(a[0]).save(os.path.join(root, "a_420.jpg"), quality=90)                     # baseline, Pillow's default 4:2:0
    Image.fromarray(a[1]).save(os.path.join(root, "b_444.jpg"), quality=85, subsampling=0)
    with open(os.path.join(root, "c_restart.jpg"), "wb") as f:
        f.write(jpeg.pillow_file(a[2], 90, "420", 4))                                           # restart interval of 4 MCUs
    Image.fromarray(a[3]).save(os.path.join(root, "d_progressive.jpg"), quality=90, progressive=True)
    Image.fromarray(a[4]).convert("L").save(os.path.join(root, "e_grey.jpg"), quality=90)
    Image.fromarray(a[5]).save(os.path.join(root, "f.png"))
    return {"a_420.jpg": "device", "b_444.jpg": "device", "c_restart.jpg": "device", "d_progressive.jpg": "host", "e_grey.jpg": "host",
            "f.png": "host"}


@pytest.mark.parametrize("with_gt", [False, True], ids=["no_gt", "gt"])
def test_every_kind_of_file_takes_its_route_and_gives_pillows_bits(tmp_path, with_gt):
    from vspbfr_amd import jpeg
    from vspbfr_amd.imageio import RestoreTestSet
    routes = _write_set(str(tmp_path / "lq"), 1)
    if with_gt:
        _write_set(str(tmp_path / "hq"), 50)
    with open(tmp_path / "lq" / "c_restart.jpg", "rb") as f:
        scan, why = jpeg.parse(f.read())
    assert why is None and scan.restart == 4 and scan.subsampling == "420"
    im_size = (32, 40)
    data = RestoreTestSet(str(tmp_path / "lq"), str(tmp_path / "hq") if with_gt else None, im_size)
    assert len(data) == 6
    how = _compare(data, with_gt, im_size, ((4, 0, 6), (1, 2, 4)), threads=3)
    assert len(how) == (12 if with_gt else 6)
    for p, v in how.items():
        assert v == routes[os.path.basename(p)], (p, v)


def test_other_decode_values_are_refused():
    from vspbfr_amd.imageio import DeviceRestoreLoader, RestoreTestSet
    data = RestoreTestSet(os.path.join(IMAGES, "lq"), None, (64, 64))
    with pytest.raises(ValueError, match="decode"):
        DeviceRestoreLoader(data, 2, DEV, decode="gpu")
    assert DeviceRestoreLoader(data, 2, DEV).decode == "host"


def test_decode_batch_pool_decodes_the_host_files(tmp_path):
    """decode_batch(pool=...): the files of the host route go through pool.map, the result is that of the call without a pool"""
    from concurrent.futures import ThreadPoolExecutor

    from vspbfr_amd import jpeg
    routes = _write_set(str(tmp_path / "set"), 7)
    paths = [str(tmp_path / "set" / n) for n in sorted(routes)]

    class Counting(ThreadPoolExecutor):
        mapped = 0

        def map(self, fn, *its):
            its = [list(i) for i in its]
            Counting.mapped += len(its[0])
            return super().map(fn, *its)
    plain = jpeg.decode_files(paths, DEV)
    with Counting(max_workers=2) as pool:
        pooled = jpeg.decode_files(paths, DEV, pool=pool)
    assert Counting.mapped == 3 and pooled[1:] == plain[1:] and torch.equal(pooled[0], plain[0])
    assert pooled[3] == [routes[n] for n in sorted(routes)]


def test_metrics_cli_device_decode_writes_the_same_directory(cli_run, capsys):  # noqa: F811
    """JPEG LQ and HQ folders: `--ingest device --decode device` against `--ingest host`, from the same seeds and checkpoints -- the
    PNGs and metrics_0.json byte for byte; --decode without --ingest device is a parser error"""
    from PIL import Image
    from vspbfr_amd import restoration_metrics
    tmp = cli_run["plain"].parents[3]
    ck = tmp / "ckpt"
    for kind in ("lq", "hq"):
        (tmp / f"{kind}_jpg").mkdir()
        for n in sorted(os.listdir(tmp / kind)):
            Image.open(tmp / kind / n).convert("RGB").save(tmp / f"{kind}_jpg" / (os.path.splitext(n)[0] + ".jpg"), quality=92)
    base = ["--batch", "2", "--ckpt", str(ck / "restoration_net.pt"), "--ddpm_ckpt", str(ck / "code_diffuser.pt"),
            "--psp_checkpoint_path", str(ck / "style_encoder_decoder.pt"), "--timesteps", "4", "--no_sample",
            "--lq_data_list", str(tmp / "lq_jpg"), "--hq_data_list", str(tmp / "hq_jpg"), "--data_name_list", "demo", "--metrics"]
    with pytest.raises(SystemExit):
        restoration_metrics.main(base + ["--eval_dir", str(tmp / "eval_refused"), "--decode", "device"])
    assert "--ingest device" in capsys.readouterr().err and not os.path.exists(tmp / "eval_refused")
    with pytest.raises(SystemExit):
        restoration_metrics.main(base + ["--eval_dir", str(tmp / "eval_refused"), "--ingest", "host", "--decode", "host"])
    dirs = {}
    for tag, extra in (("host", ["--ingest", "host"]), ("device", ["--ingest", "device", "--decode", "device"])):
        torch.manual_seed(123)
        random.seed(123)
        out = tmp / f"eval_jpg_{tag}"
        restoration_metrics.main(base + ["--eval_dir", str(out)] + extra)
        dirs[tag] = out / "restoration_net" / "0" / "demo"
    names = sorted(os.listdir(dirs["host"]))
    assert sorted(os.listdir(dirs["device"])) == names and "metrics_0.json" in names and len(names) == 10
    for n in names:
        assert (dirs["device"] / n).read_bytes() == (dirs["host"] / n).read_bytes(), n
