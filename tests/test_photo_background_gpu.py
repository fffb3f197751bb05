"""GPU checks of FacePlan.background() at upscale > 1: one ragged resize over the group, from the plan's device `photos` section into
the packed output.  Every photo equals Pillow's Image.resize((upscale w, upscale h), LANCZOS) byte for byte, whether the plan was built
from arrays or from shapes beside a device buffer; in the second case no tensor is copied to the host."""
import numpy as np
import pytest
import torch

import photo_ref as PR
import resample_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
S = 16
SHAPES = [(37, 53), (64, 48), (5, 9)]             # (h, w)


def _pil(a, f):
    from PIL import Image
    return np.asarray(Image.fromarray(a).resize((a.shape[1] * f, a.shape[0] * f), Image.Resampling.LANCZOS))


@pytest.fixture(scope="module")
def group():
    """photos, one face each, and Pillow's upscaled photos at 2 and 4 (computed once, never written to)"""
    photos = [R.test_image(w, h, seed=h * 100 + w) for h, w in SHAPES]
    faces = [(k, PR.landmarks_for(S / (0.5 * min(h, w)), 10.0 * k, (w / 2.0, h / 2.0), S)) for k, (h, w) in enumerate(SHAPES)]
    want = {f: [_pil(a, f) for a in photos] for f in (2, 4)}
    for v in want.values():
        for a in v:
            a.setflags(write=False)
    return photos, faces, want


def _flat(photos):
    return torch.from_numpy(np.concatenate([a.reshape(-1) for a in photos])).to(DEV)


@pytest.mark.parametrize("upscale", [2, 4])
def test_background_from_arrays_equals_pillow(group, upscale):
    from vspbfr_amd import photo as P
    photos, faces, want = group
    plan = P.FacePlan(photos, faces, size=S, upscale=upscale)
    out = plan.background(DEV)
    assert out.numel() == plan.out_bytes and out.dtype == torch.uint8
    for k, (got, ref) in enumerate(zip(plan.split(out), want[upscale])):
        print(f"photo {k} {SHAPES[k]} x{upscale}: differing bytes vs PIL {int((got.cpu().numpy() != ref).sum())}")
        assert np.array_equal(got.cpu().numpy(), ref), k
        assert np.array_equal(ref, R.resize(photos[k], ref.shape[1], ref.shape[0]))


@pytest.mark.parametrize("upscale", [2, 4])
def test_background_from_device_photos_copies_nothing_to_the_host(group, upscale, monkeypatch):
    from vspbfr_amd import photo as P
    photos, faces, want = group
    flat = _flat(photos)
    plan = P.FacePlan(SHAPES, faces, size=S, upscale=upscale, device_photos=flat)

    def no_copy_back(self, *a, **k):
        raise AssertionError("background() copied a tensor to the host")
    with monkeypatch.context() as m:
        m.setattr(torch.Tensor, "cpu", no_copy_back)
        out = plan.background(DEV)
        torch.cuda.synchronize()
    for k, (got, ref) in enumerate(zip(plan.split(out), want[upscale])):
        assert np.array_equal(got.cpu().numpy(), ref), k
    assert torch.equal(flat, _flat(photos))              # the source is read, not written
    # and the faces paste over it as they do over the other plan's background
    other = P.FacePlan(photos, faces, size=S, upscale=upscale)
    crops = torch.from_numpy(np.stack([R.test_image(S, S, seed=k) for k in range(len(faces))])).to(DEV)
    assert torch.equal(P.paste_faces(plan, crops, DEV), P.paste_faces(other, crops, DEV))


def test_a_photo_above_the_kernels_largest_side_takes_the_host_resize(group):
    """2 x 2050 at upscale 4 is 8 x 8200: that photo alone comes back, is resized by PIL and written into its slot, between two photos
    the kernel serves"""
    from vspbfr_amd import photo as P
    from vspbfr_amd.resample import MAX_SIDE
    photos, faces, want = group
    wide = R.test_image(2050, 2, seed=9)
    assert 4 * 2050 > MAX_SIDE
    ref = _pil(wide, 4)
    mixed = [photos[0], wide, photos[2]]
    marks = [(0, faces[0][1]), (2, faces[2][1])]
    for plan in (P.FacePlan(mixed, marks, size=S, upscale=4),
                 P.FacePlan([a.shape[:2] for a in mixed], marks, size=S, upscale=4, device_photos=_flat(mixed))):
        got = [g.cpu().numpy() for g in plan.split(plan.background(DEV))]
        assert np.array_equal(got[0], want[4][0]) and np.array_equal(got[1], ref) and np.array_equal(got[2], want[4][2])
