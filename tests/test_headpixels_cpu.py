"""What of the last layer at many pixels per image (csrc/fs_edgetrain.hip: fs_head_forward_pixels / fs_head_backward_pixels,
trainops.HeadPixelsFunction, SpatialValueNet.forward_pixels) can be checked without a GPU: the entry points exist in the header
and in the library and refuse what they do not serve before any HIP call, check_pixel_table refuses every malformed table,
forward_pixels on the host is the dense forward gathered, and the dense update IS the per-entry update: one forward_pixels +
mse_loss backward on 3 images x 5 pixels against masked_select of the dense forward on the same 15 entries as 15 replicated
images, in float64."""
import copy
import os
import re

import numpy as np
import pytest
import torch

from test_edgetrain_cpu import _aligned, _refuses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("fs_head_pixels_work_bytes", "fs_head_forward_pixels", "fs_head_backward_pixels")


def test_header_declares_and_library_exports_the_entry_points():
    from flingbot_amd import sim as fsim

    with open(os.path.join(ROOT, "include", "flingsim.h")) as fh:
        header = fh.read()
    lib = fsim.load_library()
    for name in ENTRIES:
        assert re.search(r"^(size_t|int) " + name + r"\(", header, re.M), name
        assert getattr(lib, name) is not None


def test_entry_points_refuse_what_they_do_not_serve():
    """A null pointer, a misaligned pointer, dim 32, batch 0, n_pixels 0, d_dh == d_h: FS_ERR_ARG before any HIP call (the
    pointers are host addresses that are never dereferenced), and fs_last_error() names the entry."""
    from flingbot_amd import sim as fsim

    lib = fsim.load_library()
    buf, at, off, null = _aligned()
    shape = [dict(batch=0), dict(batch=-2), dict(dim=32), dict(dim=0), dict(n=0), dict(n=-1)]

    ok = dict(h=at(0), w=at(1), offsets=at(2), pix=at(3), batch=2, n=5, dim=64, pred=at(4))
    call = lambda **a: lib.fs_head_forward_pixels(a["h"], a["w"], a["offsets"], a["pix"], a["batch"], a["n"], a["dim"], a["pred"], None)
    ptrs = ("h", "w", "offsets", "pix", "pred")
    _refuses(lib, "fs_head_forward_pixels", call, ok, shape + [{k: null} for k in ptrs] + [{k: off} for k in ptrs])

    ok = dict(h=at(0), w=at(1), offsets=at(2), pix=at(3), gpred=at(4), batch=2, n=5, dim=64, dh=at(5), dw=at(6), work=at(7))
    call = lambda **a: lib.fs_head_backward_pixels(a["h"], a["w"], a["offsets"], a["pix"], a["gpred"], a["batch"], a["n"], a["dim"],
                                                   a["dh"], a["dw"], a["work"], None)
    ptrs = ("h", "w", "offsets", "pix", "gpred", "dh", "dw", "work")
    _refuses(lib, "fs_head_backward_pixels", call, ok,
             shape + [{k: null} for k in ptrs] + [{k: off} for k in ptrs] + [dict(dh=ok["h"])])


def test_work_bytes():
    from flingbot_amd import sim as fsim

    lib = fsim.load_library()
    for args in ((0, 5, 64), (-1, 5, 64), (2, 0, 64), (2, -3, 64), (2, 5, 32), (2, 5, 0)):
        assert lib.fs_head_pixels_work_bytes(*args) == 0, args
    # one partial of 144 floats per 64 list entries, whatever the batch
    assert lib.fs_head_pixels_work_bytes(1, 1, 64) == lib.fs_head_pixels_work_bytes(9, 64, 64) == 144 * 4
    assert lib.fs_head_pixels_work_bytes(1, 65, 64) == 2 * 144 * 4
    assert lib.fs_head_pixels_work_bytes(128, 128 * 169, 64) == 338 * 144 * 4


# ---- check_pixel_table ---------------------------------------------------------------------------------------------------------
def test_check_pixel_table_accepts_empty_images_anywhere():
    from flingbot_amd.trainops import check_pixel_table

    pix = np.array([5, 9, 4095, 0, 5], np.int32)
    for offsets in ([0, 0, 2, 5], [0, 2, 2, 5], [0, 2, 5, 5], [0, 0, 0, 5], [0, 5, 5, 5]):
        if offsets in ([0, 0, 0, 5], [0, 5, 5, 5]):      # (pixel 5 twice in one image)
            with pytest.raises(ValueError, match="distinct"):
                check_pixel_table(offsets, pix, 3)
            continue
        got = check_pixel_table(np.array(offsets, np.int32), pix, 3)
        assert got.dtype == np.int64 and got.tolist() == offsets
    assert check_pixel_table([0, 0, 0, 5], np.array([5, 9, 4095, 0, 6]), 3).tolist() == [0, 0, 0, 5]
    assert check_pixel_table([0, 0], np.zeros(0, np.int32), 1).tolist() == [0, 0]          # nothing listed at all
    # the same pixel in TWO images is fine
    assert check_pixel_table([0, 1, 2], np.array([7, 7]), 2).tolist() == [0, 1, 2]
    # without a host copy of the pixels only the offsets are looked at
    assert check_pixel_table([0, 3, 3, 9], None, 3).tolist() == [0, 3, 3, 9]


@pytest.mark.parametrize("offsets,pix,batch,word", [
    ([1, 2, 3], [1, 2, 3], 2, r"offsets\[0\]"),
    ([0, 3, 2, 4], [1, 2, 3, 4], 3, "fall"),
    ([0, 2, 3], [1, 2, 3, 4], 2, "for a list of"),
    ([0, 2, 5], [1, 2, 3, 4], 2, "for a list of"),
    ([0, 2, 4], [1, 2, 3, 4096], 2, r"\[0, 4096\)"),
    ([0, 2, 4], [1, -1, 3, 4], 2, r"\[0, 4096\)"),
    ([0, 2, 4], [1, 2, 3, 3], 2, "distinct"),
    ([0, 4], [9, 2, 3, 9], 1, "distinct"),
    ([0, 2, 4], [1, 2, 3, 4], 3, "offsets are integers"),
    ([0.0, 2.0, 4.0], [1, 2, 3, 4], 2, "offsets are integers"),
    ([0, 2, 4], [1.0, 2.0, 3.0, 4.0], 2, "pixels are integers"),
    ([0, 2, 4], [[1, 2], [3, 4]], 2, "pixels are integers"),
])
def test_check_pixel_table_refuses(offsets, pix, batch, word):
    from flingbot_amd.trainops import check_pixel_table

    with pytest.raises(ValueError, match=word):
        check_pixel_table(np.array(offsets), np.array(pix), batch)


def test_check_pixel_table_checks_the_offsets_without_pixels():
    from flingbot_amd.trainops import check_pixel_table

    for bad in ([1, 2, 3], [0, 3, 2]):
        with pytest.raises(ValueError):
            check_pixel_table(bad, None, 2)


def test_function_exists_and_refuses_host_tensors():
    from flingbot_amd import nets, trainops

    fn = trainops.HeadPixelsFunction
    assert nets.HeadPixelsFunction is fn and issubclass(fn, torch.autograd.Function)
    assert isinstance(fn.n_forward, int) and isinstance(fn.n_backward, int)
    with pytest.raises(ValueError):
        fn.apply(torch.zeros(2, 16, 64, 64), torch.zeros(1, 16, 3, 3), np.array([0, 1, 2]), torch.zeros(2, dtype=torch.int32))


# ---- forward_pixels on the host ------------------------------------------------------------------------------------------------
OFFSETS = [0, 0, 3, 3, 8, 8]                                     # images 0, 2 and 4 list nothing
PIXELS = [0, 63 * 64 + 17, 20 * 64 + 40, 1, 64, 4095, 2000, 63]


@pytest.mark.parametrize("mode", ["rgb", "depth", "rgbd"])
@pytest.mark.parametrize("training", [True, False])
def test_forward_pixels_on_the_host_is_the_dense_forward_gathered(mode, training):
    """Bit for bit, with the edge switch on and off, empty images first, in the middle and last, and no Function is called."""
    from flingbot_amd import nets

    torch.manual_seed(5)
    net = nets.SpatialValueNet(rgb_only=mode == "rgb", depth_only=mode == "depth", device="cpu")
    obs = torch.rand(5, 4, 64, 64)
    pix = torch.tensor(PIXELS, dtype=torch.int32)
    image = [1, 1, 1, 3, 3, 3, 3, 3]
    calls = (nets.ConvInFunction.n_forward, nets.HeadPixelsFunction.n_forward)
    outs = []
    for edge in (False, True):
        a, b = copy.deepcopy(net).train(training), copy.deepcopy(net).train(training)
        with torch.no_grad(), nets.train_edge_hip(edge):
            got = a.forward_pixels(obs, np.array(OFFSETS), pix)
            dense = b(obs).squeeze(1)
        want = torch.stack([dense[i, p // 64, p % 64] for i, p in zip(image, PIXELS)])
        assert got.shape == (8,) and torch.equal(got, want), (mode, training, edge)
        outs.append(got)
    assert torch.equal(outs[0], outs[1])
    assert (nets.ConvInFunction.n_forward, nets.HeadPixelsFunction.n_forward) == calls
    with pytest.raises(ValueError):
        net.forward_pixels(obs, np.array([0, 0, 3, 3, 7, 7]), pix)        # the table does not cover the list
    with pytest.raises(ValueError):
        net.forward_pixels(obs, np.array([0, 3, 8]), pix)                  # nor the batch


# ---- the semantics of the update -----------------------------------------------------------------------------------------------
def test_dense_update_is_the_per_entry_update_in_float64():
    """M = 3 images x K = 5 pixels: one forward_pixels + mse_loss backward against the existing per-entry path (masked_select of
    the dense forward, one mask pixel per sample) on the same 15 entries as 15 replicated images, both on the train-mode net in
    float64.  Three pixels of every image are (0, 0), (0, 1) and (1, 0): patches that overlap at a corner.  Every image is
    replicated equally often, so the batch statistics of the two forwards coincide (BatchNorm's running_var differs by its
    N / (N - 1) factor and is not compared); loss and every parameter gradient agree within 1e-10 of the largest gradient entry."""
    from flingbot_amd import nets

    torch.manual_seed(11)
    net = nets.SpatialValueNet(rgb_only=True, device="cpu").double().train()
    net.mean, net.std = net.mean.double(), net.std.double()
    gen = torch.Generator().manual_seed(12)
    obs = torch.rand(3, 3, 64, 64, generator=gen, dtype=torch.float64)
    pixels = [[(0, 0), (0, 1), (1, 0), (30, 31), (63, 63)], [(0, 0), (0, 1), (1, 0), (17, 5), (40, 63)],
              [(0, 0), (0, 1), (1, 0), (63, 0), (12, 12)]]
    label = torch.rand(15, generator=gen, dtype=torch.float64) * 0.3 - 0.1
    flat = torch.tensor([y * 64 + x for rows in pixels for y, x in rows], dtype=torch.int32)

    dense_net = copy.deepcopy(net)
    pred = dense_net.forward_pixels(obs, np.array([0, 5, 10, 15]), flat)
    loss = torch.nn.functional.mse_loss(pred, label)
    loss.backward()

    entry_net = copy.deepcopy(net)
    mask = torch.zeros(15, 64, 64, dtype=torch.bool)
    for k, (y, x) in enumerate(p for rows in pixels for p in rows):
        mask[k, y, x] = True
    replicated = obs.repeat_interleave(5, dim=0)
    pred_entry = torch.masked_select(entry_net(replicated).squeeze(1), mask)
    loss_entry = torch.nn.functional.mse_loss(pred_entry, label)
    loss_entry.backward()

    assert pred.dtype == torch.float64 and tuple(pred.shape) == (15,)
    grads = {n: p.grad for n, p in dense_net.named_parameters() if p.grad is not None}
    grads_entry = {n: p.grad for n, p in entry_net.named_parameters() if p.grad is not None}
    assert set(grads) == set(grads_entry) and len(grads) == 2 + 16 + 2 * 17
    scale = max(float(g.abs().max()) for g in grads_entry.values())
    worst = max(float((grads[n] - grads_entry[n]).abs().max()) for n in grads)
    print(f"dense against per-entry update: loss {float(loss.detach()):.6e} / {float(loss_entry.detach()):.6e}, largest gradient entry {scale:.3e}, "
          f"largest difference {worst:.3e} = {worst / scale:.2e} of it")
    assert scale > 0 and abs(float(loss.detach()) - float(loss_entry.detach())) <= 1e-10 * scale
    assert worst <= 1e-10 * scale
