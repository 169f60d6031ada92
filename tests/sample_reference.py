"""The rules of fs_sample_actions (include/flingsim.h) restated in numpy and plain Python, independently of the kernel: the
hash in uint32, the key as two float32 operations, an exhaustive sort by (key descending, index ascending), suppression and
the on-cloth rule (tests/probe_reference.on_cloth).  Validity comes in as a table the caller fills through
ActionSelector._candidate (tests/sample_cases.py), the way tests/test_transform_winners_gpu.py::_valid uses it.

`mistake` switches ONE deliberate error on; each must change the cases that name it (tests/test_sample_actions_cpu.py):
    "noise_per_pick"      the noise is drawn again for every pick (the pick number enters the hash)
    "ties_high"           equal keys (values, for a greedy pick) go to the highest index
    "suppress_one_point"  suppression compares the first pretransform pixel only
    "fused_key"           the key is one fused multiply-add (one rounding)
    "greedy_on_cloth"     the on-cloth filter also applies to the greedy pick
    "second_point"        drag / place test their second point for cloth instead of the first"""
import numpy as np

from probe_reference import on_cloth

MISTAKES = ("noise_per_pick", "ties_high", "suppress_one_point", "fused_key", "greedy_on_cloth", "second_point")
M32 = 0xFFFFFFFF


def hash32(c, key_lo, key_hi):
    """h = c 0x9E3779B1 + key_lo 0x85EBCA77 + key_hi 0xC2B2AE3D, then the finaliser h ^= h >> 16; h *= 0x7FEB352D; h ^= h >> 15;
    h *= 0x846CA68B; h ^= h >> 16 -- wrapping uint32.  c, key_lo, key_hi: integers or integer arrays that broadcast; returns
    uint32 of the broadcast shape.  (uint64 arrays wrap modulo 2^64, which the mask reduces to modulo 2^32.)"""
    m32 = np.uint64(M32)
    c, key_lo, key_hi = (np.asarray(v).astype(np.uint64) & m32 for v in (c, key_lo, key_hi))
    h = (c * np.uint64(0x9E3779B1) + key_lo * np.uint64(0x85EBCA77) + key_hi * np.uint64(0xC2B2AE3D)) & m32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x7FEB352D)) & m32
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x846CA68B)) & m32
    h ^= h >> np.uint64(16)
    return h.astype(np.uint32)


def perturbed(values, inv_tau, noise, key, fused=False, pick=0):
    """key(c) of every candidate (values float32, flat): float32(float32(v * inv_tau) + noise[h(c) >> 16])."""
    values = np.asarray(values, np.float32)
    h = hash32(np.arange(values.size), (int(key[0]) + int(pick)) & M32, key[1])
    drawn = np.asarray(noise, np.float32)[h >> np.uint32(16)]
    with np.errstate(invalid="ignore", over="ignore"):
        if fused:   # the product of two float32 is exact in float64: one rounding at the end (up to double rounding)
            return (values.astype(np.float64) * np.float64(np.float32(inv_tau)) + drawn.astype(np.float64)).astype(np.float32)
        scaled = (values * np.float32(inv_tau)).astype(np.float32)
        return (scaled + drawn).astype(np.float32)


def cloth_table(table, depth, kinds, radius, mistake=None):
    """bool per candidate: the grasp points the primitive tests are on cloth (meaningful where table['valid'])."""
    valid, pixels = table["valid"], table["pixels"]
    out = np.zeros(valid.shape, bool)
    per_prim = valid.size // len(kinds)
    for c in np.flatnonzero(valid):
        a0, a1, b0, b1 = (int(v) for v in pixels[c])
        two = kinds[c // per_prim] in ("fling", "stretchdrag")
        if two:
            out[c] = on_cloth(depth, a1, a0, radius) and on_cloth(depth, b1, b0, radius)   # (a, b): column a, row b
        elif mistake == "second_point":
            out[c] = on_cloth(depth, b1, b0, radius)
        else:
            out[c] = on_cloth(depth, a1, a0, radius)
    return out


def _suppressed(c, prim, pixels, picks, separation, one_point):
    for pc, pprim in picks:
        if pprim != prim:
            continue
        d = np.abs(pixels[c].astype(np.int64) - pixels[pc].astype(np.int64))
        if (d[:2] if one_point else d).max() <= separation:
            return True
    return False


def sample(values, table, cloth, n_prims, k, inv_tau, noise, key, first_greedy, on_cloth_filter, separation, mistake=None):
    """One observation.  values: float32, the cropped maps values[:, :, g:-g, g:-g] flattened; table: dict(valid bool [total],
    pixels int [total, 4]); cloth: cloth_table's answer (None: r <= 0).  Returns dict(index int64 [k], value, key float32 [k],
    pixels int32 [k, 4]) and what decided the picks: tie_decided (picks with a later eligible, unsuppressed candidate of the
    same key), suppressed (candidates other than earlier picks that suppression removed in front of a pick), cloth_only
    (valid candidates with a key in front of the last pick that only the on-cloth filter excluded), tail (picks that found
    nothing)."""
    values = np.asarray(values, np.float32).ravel()
    total = values.size
    per_prim = total // n_prims
    valid = table["valid"] & ~np.isnan(values)
    pixels = table["pixels"]
    cloth_ok = np.ones(total, bool) if (cloth is None or not on_cloth_filter) else cloth
    index = np.full(k, -1, np.int64)
    value, keyo = np.zeros(k, np.float32), np.zeros(k, np.float32)
    pix = np.zeros((k, 4), np.int32)
    info = dict(tie_decided=0, suppressed=0, cloth_only=0, tail=0)
    tie = -1 if mistake == "ties_high" else 1
    picks = []

    def order_of(score, eligible):
        idx = np.flatnonzero(eligible)
        with np.errstate(invalid="ignore"):
            return idx[np.lexsort((tie * idx, -score[idx].astype(np.float64)))]

    keys = order = None
    for pick in range(k):
        greedy = bool(first_greedy) and pick == 0
        if greedy:
            eligible = valid & cloth_ok if (mistake == "greedy_on_cloth" and cloth is not None) else valid
            score, walk = values, order_of(values, eligible)
        else:
            if keys is None or mistake == "noise_per_pick":
                keys = perturbed(values, inv_tau, noise, key, fused=mistake == "fused_key",
                                 pick=pick if mistake == "noise_per_pick" else 0)
                eligible = valid & cloth_ok & ~np.isnan(keys)
                order = order_of(keys, eligible)
            score, walk = keys, order
        chosen = None
        for pos, c in enumerate(walk):
            c = int(c)
            if not greedy and _suppressed(c, c // per_prim, pixels, picks, separation, mistake == "suppress_one_point"):
                info["suppressed"] += int(all(c != pc for pc, _ in picks))
                continue
            chosen = c
            for c2 in walk[pos + 1:]:
                if score[c2] != score[c]:
                    break
                if greedy or not _suppressed(int(c2), int(c2) // per_prim, pixels, picks, separation, False):
                    info["tie_decided"] += 1
                    break
            break
        if chosen is None:
            info["tail"] = k - pick
            break
        picks.append((chosen, chosen // per_prim))
        index[pick], value[pick], keyo[pick], pix[pick] = chosen, values[chosen], score[chosen], pixels[chosen]
    if keys is not None and cloth is not None and on_cloth_filter and mistake is None:
        drawn = [c for j, (c, _) in enumerate(picks) if not (first_greedy and j == 0)]
        if drawn:
            last = drawn[-1]
            out = valid & ~cloth & ~np.isnan(keys)
            with np.errstate(invalid="ignore"):
                ahead = (keys > keys[last]) | ((keys == keys[last]) & (np.arange(total) < last))
            info["cloth_only"] = int((out & ahead).sum())
    return dict(index=index, value=value, key=keyo, pixels=pix), info
