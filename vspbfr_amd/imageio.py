"""Image I/O either side of the hot path: the test-time loader of the reference
(dataset.py:376-495 + restoration_test.py:89-94) and its PNG writer (restoration_test.py:134-157, torchvision
save_image(normalize=True, range=(-1, 1))).

Decode/resize stay on the host (PIL, exactly the reference's LANCZOS-resize-to-cover + centre crop, so pixels match);
the quantiser to 8 bits + NCHW->NHWC transpose runs on the device (vsp_quantize_u8_nhwc) so a restored batch crosses
PCIe as 0.75 MB/image of uint8 instead of 3 MB of fp32, and PNG encoding happens on a thread pool while the next batch
is already on the GPU.

`DeviceRestoreLoader` is the opt-in device ingest of the same dataset (`restoration_metrics --ingest device`): only the decode stays on the
host, on a thread pool one batch ahead; the LANCZOS resize, the crop and the normalisation run on the device (vspbfr_amd.resample,
vsp_lanczos_resize_u8) and give the bits `RestoreTestSet.__getitem__` gives.
With `decode="device"` (`--decode device`) baseline JPEG files are decoded on the device too (vspbfr_amd.jpeg) and the resize reads them
where the decoder wrote them; PNG files keep Pillow's decode.

`PngWriter(encode="device")` is the opt-in device encoder of the other end (`restoration_metrics --encode device`): row filters and deflate run
on the device (vspbfr_amd.png, vsp_png_encode_u8) and the worker threads only frame and write the files; the pixels are those of the host path.
`PngWriter.submit_photos` writes a group of whole photos from their packed buffer; with encode="device" one call of the ragged entry
(vsp_png_encode_ragged_u8, any width) codes them all (`restore_photos --png_encode device`).

`JpegWriter` writes uint8 RGB images as baseline JPEG files (`restore_photos --format jpg`): encode="device" codes them on the device
(vspbfr_amd.jpeg, vsp_jpeg_encode_u8), encode="host" hands them to Pillow at the same parameters; the two routes write equal bytes."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

IMG_EXT = (".JPG", ".jpg", ".png", ".jpeg")


def list_images(root):
    """Recursive, sorted listing with the reference's extension filter (op/utils_train.py:8-25, dataset.py:454-463)."""
    out = []
    for dp, dn, fn in os.walk(root):
        dn.sort()
        for f in fn:
            if f.endswith(IMG_EXT):
                out.append(os.path.join(dp, f))
    out.sort()
    return out


def load_rgb_u8(path):
    """An image file as the (H, W, 3) uint8 host tensor the scoring tools batch: PIL decode, converted to RGB, no resize."""
    from PIL import Image
    return torch.from_numpy(np.asarray(Image.open(path).convert("RGB"), dtype=np.uint8).copy())


def _to_tensor(img):
    """ToTensor + Normalize(0.5, 0.5) (restoration_test.py:89-94): uint8 HWC -> float32 CHW in [-1, 1]."""
    a = np.asarray(img, dtype=np.uint8)
    t = torch.from_numpy(a.copy()).permute(2, 0, 1).to(torch.float32).div_(255.0)
    return t.sub_(0.5).div_(0.5)


def _cover_and_crop(imgs, size_of, im_size):
    """LANCZOS resize so that the image `size_of` covers im_size (h, w), then the same centre crop for every image in
    `imgs` (dataset.py:410-429, 470-492: the resize target and the crop window come from ONE image's size)."""
    from PIL import Image
    w, h = size_of.size
    if h == im_size[0] and w == im_size[1]:
        return imgs
    ratio = max(1.0 * im_size[0] / h, 1.0 * im_size[1] / w)
    new_w, new_h = int(ratio * w), int(ratio * h)
    h_idx = (new_h - im_size[0]) // 2 if new_h - im_size[0] > 0 else 0
    w_idx = (new_w - im_size[1]) // 2 if new_w - im_size[1] > 0 else 0
    box = (w_idx, h_idx, int(w_idx + im_size[1]), int(h_idx + im_size[0]))
    return [im.resize((new_w, new_h), Image.Resampling.LANCZOS).crop(box) for im in imgs]


def load_image(path, im_size=(512, 512)):
    """PIL RGB -> LANCZOS resize so the image covers im_size (h, w) -> centre crop -> float32 CHW in [-1, 1]
    (dataset.py:470-495 followed by ToTensor + Normalize(0.5, 0.5), restoration_test.py:89-94)."""
    from PIL import Image
    img = Image.open(path).convert("RGB")
    return _to_tensor(_cover_and_crop([img], img, im_size)[0])


def load_pair(lq_path, hq_path, im_size=(512, 512)):
    """ImageFolder_restore_test.__getitem__ (dataset.py:408-436): the HQ image's size decides the resize and the crop of BOTH
    images (an LQ file of another size is stretched to the HQ's scaled size)."""
    from PIL import Image
    lq, hq = Image.open(lq_path).convert("RGB"), Image.open(hq_path).convert("RGB")
    lq, hq = _cover_and_crop([lq, hq], hq, im_size)
    return _to_tensor(lq), _to_tensor(hq)


class RestoreTestSet:
    """ImageFolder_restore_test / _no_gt: LQ files (and HQ files when a ground-truth root is given, paired by sorted
    order; the HQ image's size decides the resize, dataset.py:415-417)."""

    def __init__(self, lq_root, hq_root=None, im_size=(512, 512)):
        self.lq = list_images(lq_root)
        self.hq = list_images(hq_root) if hq_root not in (None, "None", "") else None
        self.im_size = im_size

    def __len__(self):
        return len(self.lq)

    def __getitem__(self, idx):
        if self.hq is None:
            return load_image(self.lq[idx], self.im_size)
        return load_pair(self.lq[idx], self.hq[idx], self.im_size)


class DeviceRestoreLoader:
    """RestoreTestSet with the resize on the device: iterates over (idx, low, gts) for the items lo..hi in batches, `low` and `gts`
    (B, 3, H, W) fp32 tensors on `device` (gts None without ground truth), bit-equal to stacking `dataset[i]`.  Only the decode
    (`Image.open(...).convert("RGB")`) stays on the host, on a pool of `threads` workers, one batch ahead of the consumer; a batch
    goes up as one pinned ragged buffer and vsp_lanczos_resize_u8 resizes, crops and normalises it (vspbfr_amd.resample).

    decode="device": the files go up as they are and baseline JPEGs are decoded on the device (vspbfr_amd.jpeg.decode_files; a PNG or
    a JPEG the decoder refuses is decoded by Pillow on the pool and copied into its slot); the resize reads the decoder's packed
    output where it lies (ResamplePlan(device_sources=...)), so no decoded pixel of a device-decoded file crosses PCIe.  Decode and
    resize of the next batch run on a stream of the loader's own, whose only host synchronisation is the decoder's status read-back;
    the consumer's stream waits on an event recorded behind the resize.  `how` maps every file read so far to its route."""

    def __init__(self, dataset, batch, device, lo=0, hi=None, threads=8, decode="host"):
        if decode not in ("host", "device"):
            raise ValueError(f"DeviceRestoreLoader: decode {decode!r}")
        self.decode, self.how, self._side = decode, {}, None
        self.ds, self.B, self.device = dataset, int(batch), torch.device(device)
        self.lo, self.hi = int(lo), len(dataset) if hi is None else int(hi)
        if self.B < 1 or not 0 <= self.lo <= self.hi <= len(dataset):
            raise ValueError(f"DeviceRestoreLoader: batch {batch}, items {lo}..{hi} of {len(dataset)}")
        self.threads = max(1, int(threads))

    @staticmethod
    def _decode(path):
        from PIL import Image
        return np.asarray(Image.open(path).convert("RGB"), dtype=np.uint8)

    def _paths(self, idx):
        return [self.ds.lq[i] for i in idx] + ([self.ds.hq[i] for i in idx] if self.ds.hq is not None else [])

    def _geometry(self, paths, shapes, n):
        """(targets, origins) of a batch whose decoded images have `shapes` = [(h, w), ...]: the LQ items first, then the HQ items"""
        from .resample import cover_geometry
        H, W = self.ds.im_size
        targets, origins = [], []
        for k, (h, w) in enumerate(shapes):
            rh, rw = shapes[n + k % n] if self.ds.hq is not None else (h, w)      # the HQ image's size decides (load_pair)
            nw, nh, box = cover_geometry(rw, rh, (H, W))
            if (nw, nh) == (rw, rh) == (W, H) and (h, w) != (H, W):
                raise ValueError(f"{paths[k]}: {w}x{h} beside a ground truth of the target size (load_pair keeps both as they are)")
            targets.append((nw, nh))
            origins.append(box[:2])
        return targets, origins

    def _host(self, pool, idx):
        """host half of a batch: decode on the pool, plan and pack the ragged upload (the LQ items first, then the HQ items)"""
        from .resample import ResamplePlan
        paths = self._paths(idx)
        arrs = list(pool.map(self._decode, paths))
        targets, origins = self._geometry(paths, [a.shape[:2] for a in arrs], len(idx))
        plan = ResamplePlan(arrs, targets, origins, self.ds.im_size)
        plan.pack()
        return plan

    def _device(self, pool, idx):
        """a whole batch on the loader's side stream: the files' bytes up, the device decode (host-route files on the pool), the
        resize from the decoder's packed buffer -> (fp32 (n, 3, H, W), the event behind it).  Called on the helper thread: the stream
        context is that thread's own, and the only thing it waits for is this stream."""
        from . import jpeg
        from .resample import ResamplePlan
        paths = self._paths(idx)
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.device)
        with torch.cuda.device(self.device), torch.cuda.stream(self._side):
            packed, shapes, offsets, how = jpeg.decode_files(paths, self.device, pool=pool)
            self.how.update(zip(paths, how))
            targets, origins = self._geometry(paths, shapes, len(idx))
            plan = ResamplePlan(shapes, targets, origins, self.ds.im_size, device_sources=(packed, offsets))
            _, out = plan.run(self.device, u8=False, f32=True)
            done = torch.cuda.Event()
            done.record(self._side)
        # packed and the work buffer were allocated on the side stream: the caching allocator hands their memory to that stream
        # alone, behind the kernels that read it, so they may be dropped here
        return out, done

    def __iter__(self):
        starts = list(range(self.lo, self.hi, self.B))
        if not starts:
            return
        batches = [list(range(s, min(s + self.B, self.hi))) for s in starts]
        with ThreadPoolExecutor(max_workers=self.threads) as pool, ThreadPoolExecutor(max_workers=1) as ahead:
            half = self._device if self.decode == "device" else self._host
            nxt = ahead.submit(half, pool, batches[0])
            for k, idx in enumerate(batches):
                got = nxt.result()
                if k + 1 < len(batches):
                    nxt = ahead.submit(half, pool, batches[k + 1])
                if self.decode == "device":
                    out, done = got
                    cur = torch.cuda.current_stream(self.device)
                    cur.wait_event(done)
                    out.record_stream(cur)          # allocated on the side stream, read on this one
                else:
                    with torch.cuda.device(self.device):
                        _, out = got.run(self.device, u8=False, f32=True)
                n = len(idx)
                yield idx, out[:n], (out[n:] if self.ds.hq is not None else None)


def output_name(eval_dir, index, rank, data_name, kind):
    """`{index:06d}_{rank}_{name}_{kind}.png`, kind in restore / low / sample / gt (restoration_test.py:140-156)."""
    return f"{str(eval_dir)}/{str(index).zfill(6)}_{str(rank)}_{data_name}_{kind}.png"


class PngWriter:
    """Device-side quantisation + asynchronous PNG encoding.  encode="host": PIL encodes on the worker threads.  encode="device": the
    row filters and the deflate stream are made on the device (vspbfr_amd.png, csrc/png.hip); the workers frame and write the files."""

    def __init__(self, workers=8, encode="host"):
        if encode not in ("host", "device"):
            raise ValueError(f"PngWriter: encode {encode!r}")
        self.pool = ThreadPoolExecutor(max_workers=workers)
        self.pending = []
        self.encode = encode

    def submit(self, batch, paths):
        """batch: (B, 3, H, W) fp32 on the device in [-1, 1] (values outside are clamped like save_image does), or the
        (B, H, W, 3) uint8 tensor such a batch quantises to.  Returns the uint8 device tensor whose bytes go to disk (what
        vspbfr_amd.metrics scores)."""
        from . import hip_ops as H
        u8 = batch if batch.dtype == torch.uint8 else H.quantize_u8_nhwc(batch.contiguous(), -1.0, 1.0)
        if self.encode == "device":
            from . import png
            if png.kernel_serves(u8.shape):
                job = png.enqueue(u8)        # encoder + asynchronous copies on the current stream; no synchronisation here
                self.pending.append(self.pool.submit(self._write, job, list(paths)))
                return u8
        host = torch.empty(u8.shape, dtype=torch.uint8, pin_memory=True)
        host.copy_(u8, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.pending.append(self.pool.submit(self._encode, host, ev, list(paths)))
        return u8

    def submit_photos(self, buffer, sizes, offsets, paths):
        """buffer: flat uint8 device tensor holding (h, w, 3) photos of `sizes` = [(h, w), ...] at the byte `offsets` (ascending, as
        photo.FacePlan.out_off lays them out), one path per photo.  encode="device": ONE ragged call codes the whole group
        (vspbfr_amd.png.enqueue_ragged, vsp_png_encode_ragged_u8) and a worker frames and writes the files; otherwise, and for a group the
        entry does not take, every photo takes the pinned copy + PIL route of submit()."""
        sizes, offsets, paths = [(int(h), int(w)) for h, w in sizes], [int(o) for o in offsets], list(paths)
        if not len(sizes) == len(offsets) == len(paths):
            raise ValueError("PngWriter.submit_photos: one size, offset and path per photo")
        if self.encode == "device" and sizes:
            from . import png
            if png.ragged_serves(sizes, 3):
                job = png.enqueue_ragged(buffer, sizes, offsets)
                self.pending.append(self.pool.submit(self._write, job, paths))
                return
        for (h, w), o, p in zip(sizes, offsets, paths):
            u8 = buffer[o:o + 3 * h * w].view(1, h, w, 3)
            host = torch.empty(u8.shape, dtype=torch.uint8, pin_memory=True)
            host.copy_(u8, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self.pending.append(self.pool.submit(self._encode, host, ev, [p]))

    @staticmethod
    def _encode(host, ev, paths):
        from PIL import Image
        ev.synchronize()
        arr = host.numpy()
        for i, p in enumerate(paths):
            Image.fromarray(arr[i]).save(p)

    @staticmethod
    def _write(job, paths):
        for p, data in zip(paths, job.files()):
            with open(p, "wb") as f:
                f.write(data)

    def drain(self):
        for f in self.pending:
            f.result()
        self.pending = []


class JpegWriter:
    """Asynchronous JPEG files of uint8 RGB images on the device.  encode="device": colour transform, DCT, quantisation and Huffman
    coding run on the device (vspbfr_amd.jpeg, csrc/jpeg.hip) and the workers copy the used bytes, frame and write; encode="host":
    Pillow encodes on the worker threads with the same quality, subsampling and restart interval, which gives the same bytes."""

    def __init__(self, workers=8, quality=90, subsampling="420", restart=None, encode="device"):
        from . import jpeg
        if encode not in ("host", "device"):
            raise ValueError(f"JpegWriter: encode {encode!r}")
        self.params = jpeg.check_params(quality, subsampling, jpeg.DEFAULT_RESTART if restart is None else restart)
        self.pool = ThreadPoolExecutor(max_workers=workers)
        self.pending = []
        self.encode = encode

    def submit(self, batch, paths):
        """batch: (B, H, W, 3) uint8 on the device, or (B, 3, H, W) fp32 in [-1, 1], quantised as PngWriter quantises it.  Returns the
        uint8 device tensor whose pixels the files hold before the lossy coding."""
        from . import hip_ops as H
        from . import jpeg
        u8 = batch if batch.dtype == torch.uint8 else H.quantize_u8_nhwc(batch.contiguous(), -1.0, 1.0)
        u8 = u8.contiguous()
        B, Hh, Ww, _ = u8.shape
        sizes = [(Hh, Ww)] * B
        if self.encode == "device" and jpeg.kernel_serves(sizes, self.params[1], self.params[2]):
            job = jpeg.enqueue(u8.reshape(-1), sizes, *self.params)       # kernels + the byte counts' copy on the current stream
            self.pending.append(self.pool.submit(self._write, job, list(paths)))
            return u8
        host = torch.empty(u8.shape, dtype=torch.uint8, pin_memory=True)
        host.copy_(u8, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.pending.append(self.pool.submit(self._encode, host, ev, list(paths), self.params))
        return u8

    @staticmethod
    def _encode(host, ev, paths, params):
        from . import jpeg
        ev.synchronize()
        arr = host.numpy()
        for i, p in enumerate(paths):
            with open(p, "wb") as f:
                f.write(jpeg.pillow_file(arr[i], *params))

    @staticmethod
    def _write(job, paths):
        for p, data in zip(paths, job.files()):
            with open(p, "wb") as f:
                f.write(data)

    def drain(self):
        for f in self.pending:
            f.result()
        self.pending = []
