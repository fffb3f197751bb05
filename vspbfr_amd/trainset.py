"""The reference's two training datasets, fed from the device degradation chain (vspbfr_amd.degrade).

  ImageFolder_restore_free_form (reference dataset.py:206-373, behind restoration_train.py:454-461): (lq1, lq2, gt), two independent
      degradations of a randomly flipped, LANCZOS-cover-resized, randomly cropped face; lq1, lq2 and gt turn grey together with
      probability 0.008.
  ImageFolder_restore (dataset.py:16-133, behind code_diffuser_train.py:365-386): (lq, gt uint8), no flip, haze or grey.

Both classes keep the reference's constructor `(root, transform=None, im_size=(256, 256))` and file listing.  `DegradeLoader` serves
batches: a keyed per-epoch shuffle sharded by rank as `data_sampler(distributed=True)` shards it (DistributedSampler: pad to a multiple
of the world size, take every world-th index), PIL decode + flip + cover resize + crop on a small thread pool, uint8 up through pinned
memory (one batch ahead of the caller), degradation on the device.  Batches are device tensors with the reference's tuple layout and ranges ([0, 1] floats, uint8 gt
for ImageFolder_restore); `*2 - 1` (and `/127.5 - 1` for a uint8 gt) maps them as the training loops do
(restoration_train.py:160-162, code_diffuser_train.py:159-161).

Every random draw of a sample is a function of (seed, epoch, dataset index, slot) (degrade.sample_rng), so a sample is read and degraded
identically whichever rank serves it at whatever world size.  The shift augmentation of the free-form class is dead code (shift_prob 0)
and left out.

`DegradeLoader(..., resize="device")` keeps only the decode on the pool: the flip, the LANCZOS cover resize and the random crop run on the
device (vspbfr_amd.resample), with the same draws in the same order, and the batches are bit-equal to the default `resize="host"`.
"""
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import degrade as D
from . import hip_ops as H
from .imageio import list_images

_SHUFFLE_SLOT = 3  # slot of the per-epoch permutation draw (index 2**63 - 1: outside every sample's counters)


class _Folder:
    params = D.DegradeParams.restore()
    n_lq = 1
    flip = False

    def __init__(self, root, transform=None, im_size=(256, 256)):
        self.root = root
        self.frame = list_images(root)
        self.transform = transform  # accepted for signature compatibility: the reference's __getitem__ never applies it
        self.im_size = (int(im_size[0]), int(im_size[1]))

    def __len__(self):
        return len(self.frame)

    def load(self, idx, rng):
        """uint8 (h, w, 3) of sample idx: decode, flip (free-form), LANCZOS resize to cover im_size, random crop (dataset.py:257-277)."""
        from PIL import Image
        img = Image.open(self.frame[idx % len(self.frame)]).convert("RGB")
        if self.flip and int(rng.integers(0, 2)) == 1:
            img = img.transpose(Image.FLIP_LEFT_RIGHT)
        w, h = img.size
        th, tw = self.im_size
        if h != th or w != tw:
            ratio = max(1.0 * th / h, 1.0 * tw / w)
            nw, nh = int(ratio * w), int(ratio * h)
            img = img.resize((nw, nh), Image.Resampling.LANCZOS)
            hr, wr = nh - th, nw - tw
            hi = int(rng.integers(0, hr + 1)) if hr > 0 else 0
            wi = int(rng.integers(0, wr + 1)) if wr > 0 else 0
            img = img.crop((wi, hi, wi + tw, hi + th))
        return np.asarray(img, dtype=np.uint8)

    def load_raw(self, idx, rng):
        """`load` up to the decode, for the device resize: (uint8 (h, w, 3) as decoded, flip, (nw, nh), (x0, y0)).  The draws from `rng`
        keep the order of `load` -- flip, crop row, crop column; the crop draws need only the resized size, which cover_geometry gives."""
        from PIL import Image
        from .resample import cover_geometry
        img = Image.open(self.frame[idx % len(self.frame)]).convert("RGB")
        flip = bool(self.flip and int(rng.integers(0, 2)) == 1)
        w, h = img.size
        th, tw = self.im_size
        nw, nh, _ = cover_geometry(w, h, self.im_size)
        hi = wi = 0
        if h != th or w != tw:
            hr, wr = nh - th, nw - tw
            hi = int(rng.integers(0, hr + 1)) if hr > 0 else 0
            wi = int(rng.integers(0, wr + 1)) if wr > 0 else 0
        return np.asarray(img, dtype=np.uint8), flip, (nw, nh), (wi, hi)

    def draws(self, epoch, idx, seed=0):
        """Host draws of one sample: (grey, [LQParams per LQ image]).  The flip / crop draws come from the same slot-0 generator in
        `load`, after the grey draw."""
        rng = D.sample_rng(seed, epoch, idx, 0)
        grey = bool(self.params.gray_prob and rng.random() < self.params.gray_prob)
        lqs = [D.sample_lq(self.params, self.im_size, D.sample_rng(seed, epoch, idx, s + 1)) for s in range(self.n_lq)]
        return grey, lqs, rng


class ImageFolder_restore_free_form(_Folder):
    """(lq1, lq2, gt) -- reference dataset.py:206-373"""
    params = D.DegradeParams.free_form()
    n_lq = 2
    flip = True


class ImageFolder_restore(_Folder):
    """(lq, gt uint8) -- reference dataset.py:16-133"""
    params = D.DegradeParams.restore()
    n_lq = 1
    flip = False


def epoch_order(n, epoch, seed=0):
    """The keyed permutation of epoch `epoch` over n samples."""
    return D.sample_rng(seed, epoch, 2 ** 63 - 1, _SHUFFLE_SLOT).permutation(n)


def shard(order, rank, world_size):
    """DistributedSampler's split: pad to a multiple of the world size with the first indices again, then every world-th index."""
    n = len(order)
    total = int(math.ceil(n / world_size)) * world_size
    order = np.concatenate([order, order[:total - n]]) if total > n else order
    return order[rank:total:world_size]


class DegradeLoader:
    """Batches of `dataset` for one rank: iterate for an endless stream (the reference's `sample_data`), or `epoch(e)` for one pass.
    Yields (lq1, lq2, gt) for ImageFolder_restore_free_form and (lq, gt uint8) for ImageFolder_restore, device tensors (B, 3, H, W)."""

    def __init__(self, dataset, batch_size, device=None, seed=0, rank=0, world_size=1, threads=4, drop_last=True, resize="host"):
        if len(dataset) == 0:
            raise ValueError(f"no images under {dataset.root}")
        if resize not in ("host", "device"):
            raise ValueError(f"resize must be 'host' or 'device' (got {resize!r})")
        self.resize = resize   # "device": the pool only decodes; flip, LANCZOS resize and crop run on the device (vspbfr_amd.resample)
        self.ds, self.B, self.seed = dataset, int(batch_size), int(seed)
        self.rank, self.world = int(rank), int(world_size)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.drop_last = drop_last
        self.pool = ThreadPoolExecutor(max_workers=max(1, int(threads)))
        self.prefetch = ThreadPoolExecutor(max_workers=1)

    def indices(self, epoch):
        return shard(epoch_order(len(self.ds), epoch, self.seed), self.rank, self.world)

    def _decode(self, epoch, idx):
        grey, lqs, rng = self.ds.draws(epoch, idx, self.seed)
        return grey, lqs, (self.ds.load(idx, rng) if self.resize == "host" else self.ds.load_raw(idx, rng))

    def _host(self, epoch, idxs):
        """host half of a batch: decode on the pool, stack into pinned memory (resize="device": pack the ragged sources and their plan)"""
        got = list(self.pool.map(lambda i: self._decode(epoch, int(i)), idxs))
        Hh, Ww = self.ds.im_size
        if self.resize == "device":
            from .resample import ResamplePlan
            raw = [g[2] for g in got]
            plan = ResamplePlan([r[0] for r in raw], [r[2] for r in raw], [r[3] for r in raw], (Hh, Ww), flips=[r[1] for r in raw])
            plan.pack()
            return got, plan
        host = torch.empty((len(got), Hh, Ww, 3), dtype=torch.uint8, pin_memory=True)
        hv = host.numpy()
        for b, (_, _, img) in enumerate(got):
            hv[b] = img
        return got, host

    def _device(self, epoch, idxs, got, host):
        """device half: upload, gt / 255, the degradation chain, grey gt where drawn"""
        B, (Hh, Ww) = len(got), self.ds.im_size
        hwc = host.to(self.device, non_blocking=True) if self.resize == "host" else host.run(self.device, u8=True)[0]
        gt = H.degrade_gt(hwc=hwc)
        n_lq = self.ds.n_lq
        lqs = [got[b][1][s] for s in range(n_lq) for b in range(B)]          # slot-major: lq1 of every sample, then lq2
        src = [b for _ in range(n_lq) for b in range(B)]
        grey = [got[b][0] for _ in range(n_lq) for b in range(B)]
        plan = D.DegradePlan(lqs, src, (Hh, Ww), B, samples=[int(idxs[b]) for b in src],
                             slots=[s + 1 for s in range(n_lq) for _ in range(B)], grey=grey)
        out = D.run_plan(plan, gt, seed=self.seed, step=epoch)
        lq = [out[s * B:(s + 1) * B] for s in range(n_lq)]
        if n_lq == 2:
            if any(g for g, _, _ in got):
                flags = torch.tensor([int(g) for g, _, _ in got], dtype=torch.int32).to(self.device, non_blocking=True)
                H.degrade_gt(src=gt, grey=flags, out=gt)
            return lq[0], lq[1], gt
        return lq[0], hwc.permute(0, 3, 1, 2).contiguous()

    def batch(self, epoch, idxs):
        """One batch of the given dataset indices."""
        return self._device(epoch, idxs, *self._host(epoch, idxs))

    def epoch(self, epoch):
        """One pass; the host half of the next batch is decoded while the caller works on the current one."""
        idx = self.indices(epoch)
        stop = len(idx) - (len(idx) % self.B if self.drop_last else 0)
        starts = list(range(0, stop, self.B))
        if not starts:
            return
        ahead = self.prefetch.submit(self._host, epoch, idx[0:self.B])
        for k, i in enumerate(starts):
            got, host = ahead.result()
            if k + 1 < len(starts):
                ahead = self.prefetch.submit(self._host, epoch, idx[starts[k + 1]:starts[k + 1] + self.B])
            yield self._device(epoch, idx[i:i + self.B], got, host)

    def __iter__(self):
        e = 0
        while True:
            yield from self.epoch(e)
            e += 1
