"""Writes tests/golden/jitter_golden.npz: what Pillow itself computes for torchvision's ColorJitter chain.

    python tests/golden/make_jitter_golden.py          (needs Pillow; build machine only)

torchvision's ColorJitter.forward on a PIL image runs, in a drawn order, functional_pil.adjust_brightness / adjust_contrast /
adjust_saturation (ImageEnhance.Brightness / Contrast / Color(img).enhance(factor)) and adjust_hue (convert('HSV'), add
uint8(hue_factor * 255) to the H plane with wrap-around, merge, convert('RGB')).  The chain below is those Pillow calls and
nothing of this repository; flingbot_amd.replay.color_jitter_host and the fs_replay_sample kernel must reproduce `outputs`
exactly (tests/test_replay_cpu.py, tests/test_replay_gpu.py).

Stored: images uint8 [I, 64, 64, 3]; image_index int32 [K]; order int32 [K, 4] (0 brightness, 1 contrast, 2 saturation,
3 hue); factors float32 [K, 4] indexed by operation; outputs uint8 [K, 64, 64, 3]; pillow_version.
"""
import itertools
import os

import numpy as np
import PIL
from PIL import Image, ImageEnhance

HERE = os.path.dirname(os.path.abspath(__file__))


def pillow_chain(img, order, factors):
    im = Image.fromarray(np.ascontiguousarray(img), "RGB")
    for op in order:
        if op == 0:
            im = ImageEnhance.Brightness(im).enhance(float(factors[0]))
        elif op == 1:
            im = ImageEnhance.Contrast(im).enhance(float(factors[1]))
        elif op == 2:
            im = ImageEnhance.Color(im).enhance(float(factors[2]))
        else:
            h, s, v = im.convert("HSV").split()
            shifted = (np.array(h, dtype=np.uint8).astype(np.int32) + int(float(factors[3]) * 255) % 256) % 256
            im = Image.merge("HSV", (Image.fromarray(shifted.astype(np.uint8), "L"), s, v)).convert("RGB")
    return np.array(im)


def images():
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[:64, :64]
    # a textured cloth-like image: a coloured patch with a weave and shading on the dark table
    weave = 18 * np.sin(xx * 1.3) * np.sin(yy * 1.1) + 0.6 * (xx - 32)
    cloth = np.zeros((64, 64, 3), np.float64)
    inside = (abs(xx - 30) < 22) & (abs(yy - 34) < 18)
    for c, base in enumerate((150, 60, 200)):
        cloth[..., c] = np.where(inside, base + weave + rng.normal(0, 4, (64, 64)), 12 + rng.normal(0, 1.5, (64, 64)))
    cloth = np.clip(cloth, 0, 255).astype(np.uint8)
    flat = np.full((64, 64, 3), (46, 46, 46), np.uint8)
    gray = np.repeat(rng.integers(90, 140, (64, 64, 1)), 3, axis=2)
    near_gray = np.clip(gray + rng.integers(-1, 2, (64, 64, 3)), 0, 255).astype(np.uint8)
    runs = rng.integers(0, 256, (64, 64, 3)).astype(np.uint8)     # runs of 0 and 255 in single channels and in all of them
    runs[:8] = 0
    runs[8:16] = 255
    runs[16:24, :, 0] = 255
    runs[24:32, :, 1] = 0
    runs[32:40, :, 2] = 255
    runs[32:40, :, 0] = 0
    noise = rng.integers(0, 256, (64, 64, 3)).astype(np.uint8)
    return np.stack([cloth, flat, near_gray, runs, noise])


def cases(n_images):
    rng = np.random.default_rng(11)
    lo, hi = np.array([0.8, 0.7, 0.5, -0.5]), np.array([1.2, 1.3, 1.5, 0.5])
    special = [lo, hi, np.array([0.8, 1.3, 0.5, 0.0]), np.array([1.2, 0.7, 1.5, 0.0]), np.array([1.0, 1.0, 1.0, 0.0]),
               np.array([1.0, 1.0, 1.0, -0.5]), np.array([1.1, 0.9, 1.2, -0.001]), np.array([0.9, 1.1, 0.7, -0.004]),
               np.array([1.05, 1.25, 0.55, -0.0039]), np.array([0.95, 0.75, 1.45, 0.0039])]
    out = []
    for k, order in enumerate(itertools.permutations(range(4))):          # all 24 orders
        f = special[k] if k < len(special) else rng.uniform(lo, hi)
        out.append((k % n_images, order, f))
    for k in range(16):                                                   # every image at the ends of the ranges again
        order = tuple(rng.permutation(4))
        f = np.where(rng.random(4) < 0.5, lo, hi) if k < 10 else rng.uniform(lo, hi)
        out.append((k % n_images, order, f))
    return out


def main():
    imgs = images()
    todo = cases(len(imgs))
    index = np.array([c[0] for c in todo], np.int32)
    order = np.array([c[1] for c in todo], np.int32)
    factors = np.array([c[2] for c in todo]).astype(np.float32)
    outputs = np.stack([pillow_chain(imgs[i], o, f) for i, o, f in zip(index, order, factors)])
    path = os.path.join(HERE, "jitter_golden.npz")
    np.savez_compressed(path, images=imgs, image_index=index, order=order, factors=factors,
                        outputs=outputs, pillow_version=np.array(PIL.__version__))
    print(path, os.path.getsize(path), "bytes;", len(todo), "cases;", len({tuple(o) for o in order}), "orders")


if __name__ == "__main__":
    main()
