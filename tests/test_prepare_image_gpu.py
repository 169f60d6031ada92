"""Device prepare_image (csrc/fs_image.hip) against the host restatement of the reference's
transform() -- scipy.ndimage.rotate (cubic spline, mode='nearest') + centre crop / replicate pad + nearest resize
(learning/nets.py:155-193).  Floating point (float64 spline arithmetic rounded to float32): tolerance 2e-6 absolute on
images in [0, 2]; the index chain (crop / pad / nearest resize / axis swaps) must agree exactly, which a wrong pixel
would violate by orders of magnitude on the random image."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 2e-6


def _policy_transforms(num_rotations=12, scales=(0.75, 1.0, 1.5, 2.0, 2.75)):
    rotations = [(2 * i / (num_rotations - 1) - 1) * 90 for i in range(num_rotations)]  # nets.py:213-214
    return [(r, s) for r in rotations for s in scales]


@pytest.mark.parametrize("size,dim", [(40, 16), (97, 64)])
def test_device_prepare_image_matches_host_transform(gpu_required, size, dim):
    from flingbot_amd import nets

    g = torch.Generator().manual_seed(size)
    img = torch.rand(4, size, size, generator=g)
    img[3] = 1.9 + 0.1 * img[3]  # depth-like channel
    yy, xx = np.mgrid[0:size, 0:size]
    img[1] = torch.tensor(((xx // 5 + yy // 7) % 2).astype(np.float32))  # hard edges: spline overshoot paths
    tf = _policy_transforms()
    ref = nets.prepare_image(img, tf, dim)                    # host path: scipy + numpy
    dev = nets.prepare_image(img.cuda(), tf, dim)             # device path
    assert dev.is_cuda and dev.shape == ref.shape == (len(tf), 4, dim, dim) and dev.dtype == torch.float32
    err = (dev.cpu() - ref).abs().max().item()
    assert err < TOL, err


def test_device_prepare_image_golden_rotations(gpu_required):
    """Against rotate_golden.npz (scipy run by tests/golden/make_golden.py): scale 1, dim == size keeps every pixel."""
    import os
    from flingbot_amd import nets

    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rotate_golden.npz"))
    img = torch.tensor(g["img"])
    size = img.shape[-1]
    angles = [float(k[4:]) for k in g.files if k.startswith("rot_")]
    dev = nets.prepare_image_device(img.cuda(), [(a, 1.0) for a in angles], size).cpu().numpy()
    for k, a in enumerate(angles):
        want = np.swapaxes(g[f"rot_{a}"], -1, 0)  # (W,H,C) -> (C,H,W), transform()'s last step
        assert np.abs(dev[k] - want).max() < TOL, a


# ---------------------------------------------------------------- against the literal chain
# The cases above compare with nets.transform, whose pixel choice (scale_window_indices) was written as "the map the kernel
# uses": an error in that map would be shared.  The cases below compare with the reference's chain written out step by step
# (learning/nets.py:144-174): rotate the (W, H, C) view, crop_center or replicate-pad to int(scale * S), nearest-resize by
# index floor(d * extent / dim), swap the axes back.  Neither nets.transform nor scale_window_indices is called.
ROTATIONS = [(2 * i / 11 - 1) * 90 for i in range(12)]                      # the fling policy's twelve
ENV_SCALES = (1.0, 1.25, 1.5, 1.75, 2.0, 2.25, 2.5, 2.75)                   # the environment's eight


class _Chain:
    """the literal chain on one image (C, S, S) float32; rotations are cached, they do not depend on the scale"""

    def __init__(self, img):
        self.plane = np.ascontiguousarray(np.asarray(img, np.float32).transpose(2, 1, 0))   # permute(2, 1, 0): (W, H, C)
        self.rot = {}

    def rotated(self, angle):
        from scipy import ndimage as nd

        if angle not in self.rot:
            self.rot[angle] = nd.rotate(self.plane, angle, reshape=False, mode='nearest')
        return self.rot[angle]

    @staticmethod
    def window(rot, scale, dim):
        S = rot.shape[0]
        new = int(scale * S)
        if scale < 1:
            start = S // 2 - new // 2
            t = rot[start:][:new][:, start:][:, :new]
        elif scale > 1:
            n = (new - S) // 2
            t = np.pad(rot, ((n, n), (n, n), (0, 0)), mode='edge')
        else:
            t = rot
        rows, cols = (np.minimum((np.arange(dim) * e) // dim, e - 1) for e in t.shape[:2])
        return t[rows][:, cols].swapaxes(-1, 0)

    def __call__(self, angle, scale, dim):
        return self.window(self.rotated(angle), scale, dim)


def _edge_scales(S):
    """scales on the edges of the crop / pad logic: int(scale * S) == S from either side, pads of 0 and 1, extents of 1,
    and the extents at which the two readings of cv2's nearest index differ (PARITY.md)"""
    return [1.0, 1 + 1e-9, 1 + 1 / S, 1 + 2 / S, 1 - 1e-9, 0.99, 0.93, 1.05, 1 / S, 1.5 / S, 2.75 * 319 / 400, 1.25 * 0.3725, 2.75]


def _test_image(C, S, seed):
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(C, S, S, generator=g)
    yy, xx = np.mgrid[0:S, 0:S]
    if C > 1:
        img[1] = torch.tensor(((xx // 5 + yy // 7) % 2).astype(np.float32))   # hard edges: spline overshoot paths
    img[C - 1] = 1.9 + 0.1 * img[C - 1]                                       # depth-like channel
    return img.numpy()


def _position_image(S):
    """img[c, y, x] names (y, x): neighbouring pixels differ by at least 2 / S^2 >= 1.25e-5 > TOL in channels 2 and 3"""
    yy, xx = np.mgrid[0:S, 0:S].astype(np.float64)
    lin = 2.0 * (yy * S + xx) / (S * S)
    return np.stack([2.0 * yy / S, 2.0 * xx / S, lin, 2.0 - lin]).astype(np.float32)


def _against_chain(img, tf, dim, chain=None):
    """max |device - chain| over the transforms (each asserted below TOL); transforms whose window is empty
    (int(scale * S) == 0, where the reference's cv2.resize raises) must be refused"""
    from flingbot_amd import nets

    chain = chain or _Chain(img)
    S = img.shape[-1]
    ok = [t for t in tf if int(t[1] * S) > 0]
    for t in tf:
        if int(t[1] * S) <= 0:
            with pytest.raises(RuntimeError, match="scale too small"):
                nets.prepare_image_device(torch.tensor(img).cuda(), [t], dim)
    dev = nets.prepare_image_device(torch.tensor(img).cuda(), ok, dim).cpu().numpy()
    assert dev.shape == (len(ok), img.shape[0], dim, dim) and dev.dtype == np.float32
    worst = 0.0
    for k, (a, s) in enumerate(ok):
        want = chain(a, s, dim)
        assert want.shape == dev[k].shape
        err = float(np.abs(dev[k] - want).max())
        assert err < TOL, (a, s, err)
        worst = max(worst, err)
    return worst


@pytest.mark.parametrize("crop", [None, 149, 319, 399])
def test_production_shape_against_the_literal_chain(gpu_required, crop):
    """The evaluation loop's call: C = 4, S = 400, dim = 64, twelve rotations x eight scale factors, multiplied by the
    adaptive crop / 400.  The measured max |diff| is printed (pytest -s)."""
    img = _test_image(4, 400, seed=400)
    f = 1.0 if crop is None else crop / 400
    worst = _against_chain(img, [(r, s * f) for r in ROTATIONS for s in ENV_SCALES], 64)
    print(f"prepare_image production shape, crop {crop}: max |diff| {worst:.2e}")


@pytest.mark.parametrize("S", [400, 97, 40])
def test_edge_scales_against_the_literal_chain(gpu_required, S):
    """Thirteen scales on the edges of the crop / pad logic at three rotations; the measured max |diff| is printed."""
    img = _test_image(4, S, seed=S + 1)
    worst = _against_chain(img, [(r, s) for r in (-90.0, ROTATIONS[6], 90.0) for s in _edge_scales(S)], 64)
    print(f"prepare_image edge scales, S {S}: max |diff| {worst:.2e}")


@pytest.mark.parametrize("C,S,dim", [(1, 97, 64), (3, 40, 16), (4, 5, 7), (2, 4, 4)])
def test_other_shapes_against_the_literal_chain(gpu_required, C, S, dim):
    img = _test_image(C, S, seed=10 * S + C)
    chain = _Chain(img)
    tf = _policy_transforms() + [(r, s) for r in (-90.0, ROTATIONS[6], 90.0) for s in _edge_scales(S)]
    worst = _against_chain(img, tf, dim, chain)
    worst = max(worst, _against_chain(img, [(ROTATIONS[4], 1.5)], dim, chain))               # T = 1
    print(f"prepare_image C {C} S {S} dim {dim}: max |diff| {worst:.2e}")


@pytest.mark.parametrize("T", [1, 40, 200])
def test_gather_grid_stride_regimes(gpu_required, T):
    """The gather runs 2048 x 256 threads over T * C * dim * dim outputs: 4096 (T = 1) and 163 840 (T = 40) leave most of
    the grid idle, 819 200 (T = 200) takes the grid-stride loop 1.56 times round."""
    rng = np.random.RandomState(T)
    img = _test_image(1, 97, seed=T)
    tf = [(float(rng.uniform(-180, 180)), float(rng.choice([0.6, 0.75, 1.0, 1.3, 2.0, 2.75]))) for _ in range(T)]
    if T == 200:
        tf = [tf[k % 20] for k in range(T)]   # twenty distinct rotations are enough work for scipy
    assert (T * 64 * 64 > 2048 * 256) == (T == 200)
    _against_chain(img, tf, 64)


def test_too_small_an_image_is_refused(gpu_required):
    from flingbot_amd import nets

    with pytest.raises(RuntimeError, match="fs_prepare_image"):
        nets.prepare_image_device(torch.rand(4, 3, 3).cuda(), [(0.0, 1.0)], 4)


@pytest.mark.parametrize("S", [400, 97, 40])
def test_position_coded_image(gpu_required, S):
    """Every pixel of the image names its own place, so ONE wrong source pixel fails by itself; at rotation 0 the expected
    output is also plain indexing of the image, without scipy."""
    img = _position_image(S)
    assert np.abs(np.diff(img[2].ravel())).min() > 5 * TOL and img.min() >= 0 and img.max() <= 2
    scales = [s for s in _edge_scales(S)]
    worst = _against_chain(img, [(r, s) for r in (0.0, -90.0, 90.0) for s in scales], 64)
    from flingbot_amd import nets
    ok = [s for s in scales if int(s * S) > 0]
    dev = nets.prepare_image_device(torch.tensor(img).cuda(), [(0.0, s) for s in ok], 64).cpu().numpy()
    plane = np.ascontiguousarray(img.transpose(2, 1, 0))
    for k, s in enumerate(ok):
        assert np.abs(dev[k] - _Chain.window(plane, s, 64)).max() < TOL, s
    print(f"prepare_image position-coded, S {S}: max |diff| {worst:.2e}")


def test_nan_pixel(gpu_required):
    """One NaN pixel in one channel: the NaN pattern equals the literal chain's (scipy's recursive prefilter spreads it over
    that channel), the other channels are untouched."""
    from flingbot_amd import nets

    img = _test_image(4, 40, seed=77)
    clean = img.copy()
    img[2, 17, 23] = np.nan
    tf = _policy_transforms() + [(0.0, 1.0), (90.0, 1 / 40)]
    dev = nets.prepare_image_device(torch.tensor(img).cuda(), tf, 16).cpu().numpy()
    chain, chain_clean = _Chain(img), _Chain(clean)
    for k, (a, s) in enumerate(tf):
        want = chain(a, s, 16)
        assert np.array_equal(np.isnan(dev[k]), np.isnan(want)), (a, s)
        assert not np.isnan(dev[k][[0, 1, 3]]).any()
        assert np.abs(dev[k][[0, 1, 3]] - chain_clean(a, s, 16)[[0, 1, 3]]).max() < TOL, (a, s)
        both = ~np.isnan(want)
        assert np.abs(dev[k][both] - want[both]).max(initial=0.0) < TOL, (a, s)
