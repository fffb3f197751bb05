"""Build a NIQE pristine model from a folder of high-quality images, with the kernel that scores (vspbfr_amd/csrc/niqe.hip).

    python -m vspbfr_amd.niqe_fit --images DIR --out params.npz [--crop_border 0] [--batch 8]

Per image the blocks whose sharpness (mean local deviation) exceeds 0.75 x the image's sharpest block are kept, as the original
fitting does; the model is the mean and covariance of their 36 features (`mu_pris_param`, `cov_pris_param`).  No model is shipped
with this package: fit one on the data your evaluation protocol names, or load a published one with `niqe.load_params`."""
import argparse

from .imageio import list_images


def image_features(paths, crop_border=0, batch=8, device="cuda"):
    """yields (features (nblk, 36), sharpness (nblk,)) as NumPy arrays per file, in order; files of one size share a launch"""
    import torch

    from . import niqe
    from .imageio import load_rgb_u8
    pend, shape = [], None

    def flush():
        if pend:
            f, s = niqe.features(torch.stack(pend).to(device, non_blocking=True), crop_border)
            f, s = f.cpu().numpy(), s.cpu().numpy()
            for k in range(len(pend)):
                yield f[k], s[k]
            pend.clear()

    for p in paths:
        img = load_rgb_u8(p)
        if shape != img.shape or len(pend) >= batch:
            yield from flush()
            shape = img.shape
        pend.append(img)
    yield from flush()


def main(argv=None):
    ap = argparse.ArgumentParser(description="Fit a NIQE pristine model (mu_pris_param, cov_pris_param) on a folder of images (MI355X)")
    ap.add_argument("--images", required=True, help="folder of high-quality images, each at least two 96 x 96 blocks")
    ap.add_argument("--out", required=True, help="the .npz to write")
    ap.add_argument("--crop_border", type=int, default=0)
    ap.add_argument("--batch", type=int, default=8)
    args = ap.parse_args(argv)
    if args.batch < 1 or args.crop_border < 0:
        ap.error("--batch must be at least 1 and --crop_border not negative")
    paths = list_images(args.images)
    if not paths:
        ap.error(f"no images in {args.images}")
    from . import niqe
    mu, cov = niqe.fit_params(image_features(paths, args.crop_border, args.batch))
    niqe.save_params(args.out, mu, cov)
    print("niqe_fit: %d images -> %s" % (len(paths), args.out))
    return mu, cov


if __name__ == "__main__":
    main()
