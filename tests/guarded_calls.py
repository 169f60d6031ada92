"""Guard bands and poisoned scratch for the device entry points of libflingsim (a helper module: no conftest, no plugin).

The suite pins what the kernels compute; this module is for what they touch.  Three pieces:

  Arena        ONE uint8 allocation that holds a slot per device argument of a call.  A slot starts on a 256-byte boundary and is
               followed AT ITS EXACT LAST BYTE + 1 by a guard; every byte of the allocation outside the slots is guard (at least
               GUARD bytes on each side of a slot) and holds a pattern that depends on its position.  `out` and `work` slots are
               pre-filled with the run's poison, `in` and `inout` slots with the caller's bytes.  After the call every guard byte
               is compared on the arena's device, and every `in` slot with what went in.
  ROLES        per stateless entry point of include/flingsim.h (the declarations that end in `void *stream)`), the role of every
               pointer parameter, by the header's parameter name.  The parameter ORDER is read from the header, so the table and
               the header cannot drift apart silently (tests/test_guarded_calls_cpu.py checks the rest).
  interposed   a context manager that puts `guarded stream_call` in the place of sim.stream_call in every flingbot_amd module
               that holds it: tensors are relocated into an arena, the real entry point runs on the slots, the arena is checked
               and the results are copied back.  The public wrappers work unchanged on top of it.

What the interposer does not see: pointers inside host tables (fs_adam_segment, fs_range_item, the panel records) pass through
as they are -- tests/test_guarded_calls_gpu.py puts fs_adam_step's arrays on an arena by hand -- and host output arrays are the
library's own copies of known size.  A relocated tensor starts on a 256-byte boundary whatever its own address was.

Poison A is 0xFF in every byte (NaN as float32 / float64, -1 as an integer); poison B is a seeded byte stream that never holds
0x00 or 0xFF.  A byte of an `out` slot that equals poison A after a run under A and poison B after the same run under B cannot
have been written by a deterministic call: `unwritten` reports those, less what the header documents as left alone.
"""
import contextlib
import ctypes as C
import os
import re
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "flingsim.h")
GUARD = 4096
ALIGN = 256
POISONS = ("A", "B")


class GuardError(AssertionError):
    """A finding of the arena: `kind` is 'guard', 'input', 'unwritten' or 'work'; `entry` the entry point, `arg` the argument
    index of the call (0 = first argument after the device), `side` 'before' / 'after' for a guard, `offset` the first bad byte
    counted from the start of the guard (before: from the guard's first byte; after: from the slot's end) or of the slot."""

    def __init__(self, kind, entry, arg, side, offset, detail=""):
        self.kind, self.entry, self.arg, self.side, self.offset = kind, entry, arg, side, offset
        where = f"argument {arg}" + (f", {side} the slot" if side else "")
        super().__init__(f"{entry}: {kind}: {where}, first changed byte at offset {offset}{detail}")


# ---- the header ------------------------------------------------------------------------------------------------------------
def parse_header(path=HEADER):
    """{entry point: [(parameter name, is_pointer, is_const)] without the trailing stream} for every declaration of the header
    that ends in `void *stream)`, and the set of names of all functions the header declares."""
    with open(path) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    declared, entries = set(), {}
    for m in re.finditer(r"\b(fs_\w+)\s*\(([^()]*)\)\s*;", text):
        name, params = m.group(1), " ".join(m.group(2).split())
        declared.add(name)
        if not params.endswith("void *stream"):
            continue
        out = []
        for p in params.split(",")[:-1]:
            p = p.strip()
            out.append((re.search(r"(\w+)$", p).group(1), "*" in p, p.startswith("const ")))
        entries[name] = out
    return entries, declared


def _dims(*names):
    return lambda a: tuple(int(a[n]) for n in names)


def _lattice_dims(a):
    m = int(a["m"])
    req = a["requests"]
    address = req if isinstance(req, int) else C.cast(req, C.c_void_p).value
    table = (C.c_int * (8 * m)).from_address(address)
    cells = max(table[8 * k + 6] * table[8 * k + 7] for k in range(m))
    return int(a["n"]), int(a["n_transforms"]), m, int(cells)


def _unowned_labels(a):
    """Byte mask of d_dpred [labels] float32: the entries no clamped image of d_offsets owns."""
    off = a["d_offsets"].detach().cpu().to(torch.int64).tolist()
    L = int(a["labels"])
    owned = torch.zeros(L, dtype=torch.bool)
    for b in range(int(a["images"])):
        begin = min(max(off[b], 0), L)
        end = min(min(max(off[b + 1], begin), L), begin + 4096)
        owned[begin:end] = True
    return (~owned).repeat_interleave(4)


def _unread_rows(row_bytes):
    def mask(a):
        index = a["d_table"].detach().cpu().view(-1, 9)[:, 0].to(torch.int64)
        bad = (index < 0) | (index >= int(a["n_samples"]))
        return bad.repeat_interleave(int(row_bytes(a)))
    return mask


class Role:
    """kind: 'in' | 'out' | 'inout' | 'work'.  work: (size function of the header, call arguments -> its arguments).
    left_alone: (the header's sentence, call arguments -> byte mask of the output the call documents as not written).
    optional: the header's sentence that allows a null pointer."""

    def __init__(self, kind, work=None, left_alone=None, optional=None):
        self.kind, self.work, self.left_alone, self.optional = kind, work, left_alone, optional


IN, OUT, INOUT = Role("in"), Role("out"), Role("inout")


def WORK(size_function, dims):
    return Role("work", work=(size_function, dims))


_ACTION = dict(d_values=IN, primitive_kinds=IN, transform_mats=IN, d_depth=IN, pose_matrix=IN, left_arm_base=IN,
               right_arm_base=IN)
_MAP_DPRED = "a d_dpred entry that no clamped image owns is left unwritten"
_LIST_DPRED = "an entry no image owns is not written"
_REPLAY_ROW = "A table row whose index is outside [0, n_samples) reads nothing and leaves its outputs unwritten."

ROLES = {
    "fs_prepare_image": dict(d_img=IN, matrix=IN, offset=IN, scale=IN, d_out=OUT,
                             d_work=WORK("fs_prepare_image_work_bytes", _dims("channels", "size", "n_transforms"))),
    "fs_select_action": dict(_ACTION, best_index_out=OUT, best_value_out=OUT,
                             d_work=WORK("fs_select_action_work_bytes", _dims("n_transforms"))),
    "fs_transform_winners": dict(_ACTION, index_out=OUT, value_out=OUT,
                                 d_work=WORK("fs_transform_winners_work_bytes", _dims("n", "n_primitives", "n_transforms"))),
    "fs_lattice_actions": dict(_ACTION, requests=IN, code_out=OUT, value_out=OUT,
                               d_work=WORK("fs_lattice_actions_work_bytes", _lattice_dims)),
    "fs_sample_actions": dict(_ACTION, d_noise=IN, sample_keys=IN, index_out=OUT, value_out=OUT, key_out=OUT, pix_out=OUT,
                              d_work=WORK("fs_sample_actions_work_bytes",
                                          _dims("n", "n_primitives", "n_transforms", "obs_dim", "pix_grasp_dist", "k"))),
    "fs_value_net_forward": dict(d_params=IN, d_obs=IN, d_out=OUT, d_work=WORK("fs_value_net_work_bytes", _dims("batch", "size"))),
    "fs_conv16_forward": dict(d_x=IN, d_w=IN, d_y=OUT),
    "fs_conv16_wgrad": dict(d_x=IN, d_g=IN, d_dw=OUT, d_work=WORK("fs_conv16_work_bytes", _dims("batch", "dim"))),
    "fs_bn16_forward": dict(d_x=IN, d_residual=Role("in", optional="(+ d_residual when it is given)"), d_gamma=IN, d_beta=IN,
                            d_running_mean=Role("inout", optional="When d_running_mean and d_running_var are given (both or "
                                                                  "neither) they are updated IN PLACE"),
                            d_running_var=Role("inout", optional="When d_running_mean and d_running_var are given (both or "
                                                                 "neither) they are updated IN PLACE"),
                            d_y=OUT, d_save_mean=OUT, d_save_invstd=OUT, d_work=WORK("fs_bn16_work_bytes", _dims("batch", "dim"))),
    "fs_bn16_backward": dict(d_x=IN, d_y=IN, d_dy=IN, d_gamma=IN, d_save_mean=IN, d_save_invstd=IN, d_dx=OUT,
                             d_dresidual=Role("out", optional="d_dresidual = dz when it is given (null: no residual was given "
                                                              "to the forward)"),
                             d_dgamma=OUT, d_dbeta=OUT, d_work=WORK("fs_bn16_work_bytes", _dims("batch", "dim"))),
    "fs_convin_forward": dict(d_x=IN, d_w=IN, d_y=OUT),
    "fs_convin_wgrad": dict(d_x=IN, d_g=IN, d_dw=OUT, d_work=WORK("fs_convin_work_bytes", _dims("channels", "batch", "dim"))),
    "fs_head_forward": dict(d_h=IN, d_w=IN, d_pix=IN, d_pred=OUT),
    "fs_head_backward": dict(d_h=IN, d_w=IN, d_pix=IN, d_gpred=IN, d_dh=OUT, d_dw=OUT),
    "fs_head_forward_pixels": dict(d_h=IN, d_w=IN, d_offsets=IN, d_pix=IN, d_pred=OUT),
    "fs_head_backward_pixels": dict(d_h=IN, d_w=IN, d_offsets=IN, d_pix=IN, d_gpred=IN, d_dh=OUT, d_dw=OUT,
                                    d_work=WORK("fs_head_pixels_work_bytes", _dims("batch", "n_pixels", "dim"))),
    "fs_adam_step": dict(segments=IN),   # the four arrays of a segment are reachable only through the table: the test uses the arena
    "fs_replay_sample": dict(d_obs=IN, d_masks=IN, d_labels=IN, d_table=IN,
                             d_out_obs=Role("out", left_alone=(_REPLAY_ROW, _unread_rows(
                                 lambda a: 4 * int(a["channels"]) * int(a["size"]) ** 2))),
                             d_out_mask=Role("out", left_alone=(_REPLAY_ROW, _unread_rows(lambda a: int(a["size"]) ** 2))),
                             d_out_label=Role("out", left_alone=(_REPLAY_ROW, _unread_rows(lambda a: 4)))),
    "fs_group_loss": dict(d_pred=IN, d_label=IN, d_bounds=IN, d_dpred=OUT, d_stats=OUT),
    "fs_map_loss": dict(d_pred=IN, d_label=IN, d_offsets=IN, d_dpred=Role("out", left_alone=(_MAP_DPRED, _unowned_labels)),
                        d_stats=OUT, d_table=OUT, d_work=WORK("fs_map_loss_work_bytes", _dims("images", "labels"))),
    "fs_map_list_loss": dict(d_pred=IN, d_label=IN, d_offsets=IN, d_dpred=Role("out", left_alone=(_LIST_DPRED, _unowned_labels)),
                             d_stats=OUT, d_table=OUT, d_work=WORK("fs_map_list_work_bytes", _dims("images", "labels"))),
    "fs_map_list_sweep": dict(d_pred=IN, d_label=IN, d_offsets=IN, temperatures=IN, d_curve=OUT, d_rows=OUT, d_images=OUT,
                              d_work=WORK("fs_map_list_sweep_work_bytes", _dims("images", "labels", "n_temperatures"))),
    "fs_map_score": dict(d_value=IN, d_pix=IN, d_label=IN, d_offsets=IN, d_rows=OUT),
    "fs_value_range": dict(items=IN, d_out=OUT),
    "fs_action_panels": dict(table=IN, d_out=OUT, d_work=WORK("fs_action_panels_work_bytes", _dims("n_actions"))),
    "fs_lane_panels": dict(table=IN, d_out=OUT, d_work=WORK("fs_lane_panels_work_bytes", _dims("n_records"))),
    "fs_probe_panels": dict(table=IN, d_out=OUT, d_work=WORK("fs_probe_panels_work_bytes", _dims("n_records"))),
}
OBSERVE_ENTRIES = ("fs_observe", "fs_observe_batch", "fs_observe_frames")   # context calls: the tests drive them on an arena


def left_alone_exceptions():
    """[(entry point, parameter, the header's sentence)] of every documented exception the table lists."""
    out = []
    for entry, roles in ROLES.items():
        for param, role in roles.items():
            if role.left_alone:
                out.append((entry, param, role.left_alone[0]))
            if role.optional:
                out.append((entry, param, role.optional))
    return out


# ---- bytes -----------------------------------------------------------------------------------------------------------------
def byte_view(t):
    """The memory of a contiguous tensor as a uint8 [nbytes] tensor that shares it."""
    if not t.is_contiguous():
        raise ValueError("guarded call: a device argument must be contiguous")
    nbytes = t.numel() * t.element_size()
    return torch.empty(0, dtype=torch.uint8, device=t.device).set_(t.untyped_storage(), t.storage_offset() * t.element_size(),
                                                                    (nbytes,), (1,))


def guard_pattern(n, device):
    """Guard byte at arena offset o: fixed, non-trivial, depends on the position (and differs between neighbouring 256-byte rows)."""
    o = torch.arange(n, dtype=torch.int64, device=device)
    return ((o * 131 + (o >> 8) * 29 + (o >> 16) * 7 + 0x5A) & 0xFF).to(torch.uint8)


def poison_bytes(which, n, seed, device):
    if which == "A":
        return torch.full((n,), 0xFF, dtype=torch.uint8, device=device)
    if which != "B":
        raise ValueError(f"poison pattern {which!r}: 'A' or 'B'")
    g = torch.Generator().manual_seed(0x5EED + 7919 * int(seed))
    return torch.randint(1, 255, (n,), generator=g, dtype=torch.uint8).to(device)   # 1 .. 254: never 0x00, never 0xFF


class Slot:
    def __init__(self, arg, nbytes, role, source=None, keep=None):
        """arg: the argument index it reports under; nbytes: exact size; role: 'in' | 'out' | 'inout' | 'work'; source: uint8
        tensor of the caller's bytes (in / inout always; out: only read under `keep`); keep: bool byte mask of an `out` slot
        that takes the caller's bytes instead of poison (documented as left alone)."""
        self.arg, self.nbytes, self.role, self.source, self.keep = arg, int(nbytes), role, source, keep
        self.start = None


class Arena:
    """One uint8 allocation on `device` with a slot per entry of `slots` (see the module docstring)."""

    def __init__(self, device, slots, poison="A", entry="arena", seed=0):
        self.device, self.slots, self.poison, self.entry = torch.device(device), list(slots), poison, entry
        probe_size = GUARD + ALIGN + sum(s.nbytes + 2 * GUARD + ALIGN for s in self.slots)
        self.buffer = torch.empty(probe_size, dtype=torch.uint8, device=self.device)
        base = self.buffer.data_ptr()
        cursor = 0
        for s in self.slots:
            cursor += GUARD
            cursor += (-(base + cursor)) % ALIGN
            s.start = cursor
            cursor += s.nbytes + GUARD
        self.size = cursor
        assert self.size <= probe_size
        self.buffer = self.buffer[:self.size]
        self.pattern = guard_pattern(self.size, self.device)
        self.buffer.copy_(self.pattern)
        self.is_guard = torch.ones(self.size, dtype=torch.bool, device=self.device)
        self.filled = {}
        for k, s in enumerate(self.slots):
            self.is_guard[s.start:s.start + s.nbytes] = False
            view = self.view(k)
            if s.role in ("in", "inout"):
                view.copy_(s.source)
                if s.role == "in":
                    self.filled[k] = view.clone()
            else:
                fill = poison_bytes(poison, s.nbytes, seed * 1000 + k, self.device)
                if s.keep is not None and s.source is not None:
                    keep = s.keep.to(self.device)
                    fill = torch.where(keep, s.source.to(self.device), fill)
                view.copy_(fill)
                self.filled[k] = fill

    def view(self, k):
        s = self.slots[k]
        return self.buffer[s.start:s.start + s.nbytes]

    def typed(self, k, dtype, shape=None):
        t = self.view(k).view(dtype)
        return t if shape is None else t.view(shape)

    def ptr(self, k):
        return self.buffer.data_ptr() + self.slots[k].start

    def sync(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    def check_guards(self):
        self.sync()
        bad = (self.buffer != self.pattern) & self.is_guard
        if not bool(bad.any()):
            return
        at = int(torch.nonzero(bad)[0])
        # the guard bytes in front of slot k run from the previous slot's end + GUARD (or 0) to its start
        for k, s in enumerate(self.slots):
            end = s.start + s.nbytes
            front = 0 if k == 0 else self.slots[k - 1].start + self.slots[k - 1].nbytes + GUARD
            if front <= at < s.start:
                raise GuardError("guard", self.entry, s.arg, "before", at - front, f" ({s.start - at} bytes in front of the slot)")
            if end <= at < end + GUARD:
                raise GuardError("guard", self.entry, s.arg, "after", at - end, f" (slot of {s.nbytes} bytes)")
        raise AssertionError(f"{self.entry}: guard byte {at} changed outside every band")

    def check_inputs(self):
        self.sync()
        for k, s in enumerate(self.slots):
            if s.role == "in":
                bad = self.view(k) != self.filled[k]
                if bool(bad.any()):
                    raise GuardError("input", self.entry, s.arg, None, int(torch.nonzero(bad)[0]), " of a const argument")

    def check(self):
        self.check_guards()
        self.check_inputs()

    def still_poisoned(self, k):
        """bool byte mask of an out / work slot: the bytes that hold what they were pre-filled with."""
        return self.view(k) == self.filled[k]


def unwritten(entry, slots_a, still_a, still_b, skip=None):
    """Raise for the first byte of an `out` slot that kept poison A in one run and poison B in the other.  still_*: {slot index:
    bool byte mask}; skip: {slot index: bool byte mask of bytes documented as left alone}."""
    for k in sorted(still_a):
        both = still_a[k] & still_b[k]
        if skip and skip.get(k) is not None:
            both = both & ~skip[k].to(both.device)
        if bool(both.any()):
            raise GuardError("unwritten", entry, slots_a[k].arg, None, int(torch.nonzero(both)[0]), " of an output")


# ---- the interposer ----------------------------------------------------------------------------------------------------------
class Interposer:
    def __init__(self, poison, lib):
        self.poison, self.lib = poison, lib
        self.counts, self.records = {}, []
        self.entries, _ = parse_header()
        self.real = None

    def work_bytes(self, name, named):
        function, dims = ROLES[name]["d_work"].work
        return int(getattr(self.lib, function)(*dims(named)))

    def __call__(self, name, device, *args):
        params = self.entries.get(name)
        if params is None or name not in ROLES:
            raise AssertionError(f"{name}: no role table entry (tests/guarded_calls.py ROLES)")
        if len(args) != len(params):
            raise AssertionError(f"{name}: {len(args)} arguments for the header's {len(params)}")
        named = {p[0]: a for p, a in zip(params, args)}
        roles = ROLES[name]
        # tensors whose storage ranges overlap share one slot (its role: the strongest of theirs; its bytes: the union)
        groups = []
        for k, a in enumerate(args):
            if not isinstance(a, torch.Tensor):
                continue
            role = roles[params[k][0]]
            if role.kind == "work":
                need = self.work_bytes(name, named)
                have = a.numel() * a.element_size()
                if have < need:
                    raise GuardError("work", name, k, None, have, f": the wrapper passes {have} bytes of scratch, "
                                     f"{role.work[0]} asks for {need}")
                groups.append(dict(args=[k], lo=None, hi=None, kind="work", nbytes=need, role=role))
                continue
            view = byte_view(a)
            lo, hi = view.data_ptr(), view.data_ptr() + view.numel()
            for g in groups:
                if g["kind"] != "work" and g["storage"] == a.untyped_storage().data_ptr() and lo < g["hi"] and g["lo"] < hi:
                    g["args"].append(k)
                    g["lo"], g["hi"] = min(g["lo"], lo), max(g["hi"], hi)
                    g["kind"] = "inout" if (g["kind"], role.kind) != ("in", "in") else "in"
                    g["role"] = None
                    break
            else:
                groups.append(dict(args=[k], lo=lo, hi=hi, kind=role.kind, storage=a.untyped_storage().data_ptr(), tensor=a,
                                   role=role))
        slots, skips = [], {}
        for j, g in enumerate(groups):
            if g["kind"] == "work":
                slots.append(Slot(g["args"][0], g["nbytes"], "work"))
                continue
            t = g["tensor"]
            source = torch.empty(0, dtype=torch.uint8, device=t.device).set_(
                t.untyped_storage(), g["lo"] - t.untyped_storage().data_ptr(), (g["hi"] - g["lo"],), (1,))
            g["bytes"] = source
            keep = None
            if g["kind"] == "out" and g["role"] is not None and g["role"].left_alone:
                keep = g["role"].left_alone[1](named)
                skips[j] = keep
            slots.append(Slot(g["args"][0], g["hi"] - g["lo"], g["kind"], source, keep))
        dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        arena = Arena(next((g["tensor"].device for g in groups if g["kind"] != "work"), dev), slots, self.poison, name,
                      seed=len(self.records))
        moved = list(args)
        for j, g in enumerate(groups):
            for k in g["args"]:
                if g["kind"] == "work":
                    moved[k] = arena.view(j)
                else:
                    offset = byte_view(args[k]).data_ptr() - g["lo"]
                    moved[k] = arena.view(j)[offset:offset + args[k].numel() * args[k].element_size()]
        self.counts[name] = self.counts.get(name, 0) + 1
        self.real(name, device, *moved)
        arena.check()
        still = {}
        for j, g in enumerate(groups):
            if g["kind"] in ("out", "inout"):
                g["bytes"].copy_(arena.view(j))
            if g["kind"] == "out":
                still[j] = arena.still_poisoned(j)
        self.records.append((name, slots, still, skips))


def assert_outputs_written(run_a, run_b):
    """The two interposed runs of one case, under poison A and poison B: same calls, and no output byte kept both poisons."""
    assert [r[0] for r in run_a.records] == [r[0] for r in run_b.records], "the two runs made different calls"
    for (name, slots, still_a, skips), (_, _, still_b, _) in zip(run_a.records, run_b.records):
        unwritten(name, slots, still_a, still_b, skips)


MODULES = ("sim", "action", "nets", "trainops", "report", "replay", "train")


@contextlib.contextmanager
def interposed(poison):
    """Replace stream_call in every flingbot_amd module that holds it; yields the Interposer (counts, records)."""
    import importlib

    for m in MODULES:
        importlib.import_module("flingbot_amd." + m)
    sim = sys.modules["flingbot_amd.sim"]
    real = sim.stream_call
    guard = Interposer(poison, sim.load_library())
    guard.real = real
    patched = []
    for name, module in list(sys.modules.items()):
        if module is not None and (name == "flingbot_amd" or name.startswith("flingbot_amd.")) \
                and getattr(module, "stream_call", None) is real:
            module.stream_call = guard
            patched.append(module)
    try:
        yield guard
    finally:
        for module in patched:
            module.stream_call = real
