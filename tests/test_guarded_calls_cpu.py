"""The guard-band helper itself, without a GPU: the role table against include/flingsim.h, and the arena on CPU tensors with
mistakes planted by plain torch writes (no kernel is made to misbehave anywhere)."""
import re

import pytest
import torch

import guarded_calls as gc


# ---- the role table ----------------------------------------------------------------------------------------------------------
def test_every_stream_entry_point_has_a_role_for_every_pointer():
    entries, declared = gc.parse_header()
    assert len(entries) == 27, sorted(entries)
    assert set(entries) == set(gc.ROLES), (sorted(set(entries) - set(gc.ROLES)), sorted(set(gc.ROLES) - set(entries)))
    for name, params in entries.items():
        roles = gc.ROLES[name]
        pointers = [p for p, is_pointer, _ in params if is_pointer]
        assert sorted(pointers) == sorted(roles), (name, sorted(set(pointers) ^ set(roles)))
        for p, is_pointer, is_const in params:
            if not is_pointer:
                continue
            kind = roles[p].kind
            assert kind in ("in", "out", "inout", "work"), (name, p, kind)
            assert (kind == "in") == is_const, f"{name}: {p} is {'const' if is_const else 'not const'} and has role {kind}"
            assert (kind == "work") == (p == "d_work"), (name, p, kind)
            if kind == "work":
                function, dims = roles[p].work
                assert re.fullmatch(r"fs_\w+_work_bytes", function) and function in declared, (name, function)
                assert callable(dims)


def test_a_new_entry_point_or_a_missing_row_is_noticed(tmp_path):
    with open(gc.HEADER) as f:
        text = f.read()
    grown = tmp_path / "flingsim.h"
    grown.write_text(text.replace("#ifdef __cplusplus\n}", "int fs_new_thing(const float *d_a, float *d_b, void *stream);\n"
                                                           "#ifdef __cplusplus\n}", 1))
    entries, _ = gc.parse_header(str(grown))
    assert set(entries) - set(gc.ROLES) == {"fs_new_thing"}
    assert entries["fs_new_thing"] == [("d_a", True, True), ("d_b", True, False)]
    fewer = dict(gc.ROLES)
    del fewer["fs_map_score"]
    assert set(gc.parse_header()[0]) - set(fewer) == {"fs_map_score"}


def test_work_sizes_take_the_calls_own_dimensions():
    named = dict(batch=9, dim=64, size=64, channels=3, n_pixels=65, images=5, labels=4360, n_temperatures=33, n=3, n_primitives=2,
                 n_transforms=6, obs_dim=27, pix_grasp_dist=2, k=16, n_actions=4, n_records=3)
    for name, roles in gc.ROLES.items():
        if "d_work" in roles and name != "fs_lattice_actions":
            dims = roles["d_work"].work[1](named)
            assert dims and all(isinstance(v, int) for v in dims), name
    assert gc.ROLES["fs_map_list_sweep"]["d_work"].work[1](named) == (5, 4360, 33)
    import ctypes as C

    table = (C.c_int * 16)(0, 0, 0, 1, 1, 2, 3, 5, 1, 0, 1, 0, 0, 1, 7, 2)
    assert gc._lattice_dims(dict(n=2, n_transforms=4, m=2, requests=C.addressof(table))) == (2, 4, 2, 15)


def test_left_alone_exceptions_quote_the_header():
    with open(gc.HEADER) as f:
        flat = " ".join(f.read().split())
    listed = gc.left_alone_exceptions()
    assert {(e, p) for e, p, _ in listed} >= {("fs_map_loss", "d_dpred"), ("fs_map_list_loss", "d_dpred"),
                                              ("fs_replay_sample", "d_out_obs"), ("fs_bn16_forward", "d_residual"),
                                              ("fs_bn16_backward", "d_dresidual")}
    for entry, param, sentence in listed:
        assert " ".join(sentence.split()) in flat, (entry, param, sentence)
    off = torch.tensor([0, 1, 3, 260, 260, 4360], dtype=torch.int32)
    mask = gc._unowned_labels(dict(d_offsets=off, images=5, labels=4360))
    assert mask.shape == (4 * 4360,) and torch.nonzero(mask).flatten().tolist() == list(range(4 * 4356, 4 * 4360))


# ---- the arena ---------------------------------------------------------------------------------------------------------------
SIZES = (1, 7, 4099)


def _arena(poison, device="cpu"):
    g = torch.Generator().manual_seed(5)
    sources = [torch.randint(0, 256, (n,), generator=g, dtype=torch.uint8) for n in SIZES]
    slots = [gc.Slot(3, SIZES[0], "in", sources[0]), gc.Slot(5, SIZES[1], "out"), gc.Slot(6, SIZES[2], "in", sources[2]),
             gc.Slot(8, 12, "work"), gc.Slot(9, 40, "out")]
    return gc.Arena(device, slots, poison, "fs_selftest"), sources


def _honest_call(arena):
    """What a correct entry point does, in torch writes: every byte of both outputs, some of the scratch, no input."""
    arena.view(1).copy_(torch.arange(7, dtype=torch.uint8) + arena.view(0)[0])
    arena.view(3)[:8] = 3
    arena.typed(4, torch.float32).copy_(torch.arange(10, dtype=torch.float32) * arena.view(2)[:10].float())


@pytest.mark.parametrize("poison", gc.POISONS)
def test_layout_and_clean_run(poison):
    arena, sources = _arena(poison)
    ends = [0]
    for k, s in enumerate(arena.slots):
        assert (arena.buffer.data_ptr() + s.start) % gc.ALIGN == 0 and arena.ptr(k) == arena.buffer.data_ptr() + s.start
        assert s.start - ends[-1] >= gc.GUARD
        ends.append(s.start + s.nbytes)
        assert not arena.is_guard[s.start:s.start + s.nbytes].any()
        assert arena.is_guard[s.start - gc.GUARD:s.start].all() and arena.is_guard[ends[-1]:ends[-1] + gc.GUARD].all()
    assert arena.size == ends[-1] + gc.GUARD
    assert int(arena.is_guard.sum()) == arena.size - sum(s.nbytes for s in arena.slots)
    pattern = gc.guard_pattern(arena.size, "cpu")
    assert torch.equal(arena.buffer[arena.is_guard], pattern[arena.is_guard])
    assert len(set(pattern[:4096].tolist())) > 200 and not torch.equal(pattern[:256], pattern[256:512])   # non-trivial, positional
    assert torch.equal(arena.view(0), sources[0]) and torch.equal(arena.view(2), sources[2])
    fill = arena.view(1).clone()
    assert (fill == 0xFF).all() if poison == "A" else ((fill != 0) & (fill != 0xFF)).all()
    assert arena.still_poisoned(1).all() and arena.still_poisoned(3).all()
    _honest_call(arena)
    arena.check()


def test_pattern_b_is_seeded_and_nonzero():
    a, b = gc.poison_bytes("B", 5000, 1, "cpu"), gc.poison_bytes("B", 5000, 1, "cpu")
    assert torch.equal(a, b) and not torch.equal(a, gc.poison_bytes("B", 5000, 2, "cpu"))
    assert int(a.min()) >= 1 and int(a.max()) <= 254 and len(set(a.tolist())) > 200
    with pytest.raises(ValueError):
        gc.poison_bytes("C", 1, 0, "cpu")


def test_a_byte_in_front_of_a_slot_is_reported():
    arena, _ = _arena("A")
    _honest_call(arena)
    s, before = arena.slots[2], arena.slots[1]
    arena.buffer[s.start - 1] ^= 0x01
    with pytest.raises(gc.GuardError) as e:
        arena.check_guards()
    front = before.start + before.nbytes + gc.GUARD
    assert (e.value.kind, e.value.entry, e.value.arg, e.value.side) == ("guard", "fs_selftest", 6, "before")
    assert e.value.offset == s.start - 1 - front
    assert "fs_selftest" in str(e.value) and "argument 6" in str(e.value) and "before" in str(e.value)


def test_a_byte_after_the_exact_end_of_an_odd_slot_is_reported():
    arena, _ = _arena("B")
    _honest_call(arena)
    s = arena.slots[2]
    assert s.nbytes == 4099 and (s.start + s.nbytes) % 4 != 0   # the guard does not start at a rounded size
    arena.buffer[s.start + s.nbytes] ^= 0x80
    with pytest.raises(gc.GuardError) as e:
        arena.check_guards()
    assert (e.value.kind, e.value.arg, e.value.side, e.value.offset) == ("guard", 6, "after", 0)
    arena.buffer[s.start + s.nbytes] ^= 0x80
    arena.check()
    first = arena.slots[0]
    arena.buffer[first.start + 1 + 100] = arena.buffer[first.start + 1 + 100] + 1   # behind the 1-byte slot
    with pytest.raises(gc.GuardError) as e:
        arena.check_guards()
    assert (e.value.arg, e.value.side, e.value.offset) == (3, "after", 100)


def test_a_changed_input_is_reported():
    arena, _ = _arena("A")
    _honest_call(arena)
    arena.view(2)[4098] ^= 0x10
    arena.check_guards()
    with pytest.raises(gc.GuardError) as e:
        arena.check()
    assert (e.value.kind, e.value.arg, e.value.side, e.value.offset) == ("input", 6, None, 4098)


def test_an_output_element_that_is_never_written_is_reported():
    stills = []
    for poison in gc.POISONS:
        arena, _ = _arena(poison)
        _honest_call(arena)
        stills.append((arena, {k: arena.still_poisoned(k) for k, s in enumerate(arena.slots) if s.role == "out"}))
    (arena_a, still_a), (_, still_b) = stills
    gc.unwritten("fs_selftest", arena_a.slots, still_a, still_b)          # the honest call wrote everything
    stills = []
    for poison in gc.POISONS:
        arena, _ = _arena(poison)
        kept = arena.typed(4, torch.float32)[7].clone()
        _honest_call(arena)
        arena.typed(4, torch.float32)[7] = kept                            # as if element 7 had been skipped
        arena.check()
        stills.append({k: arena.still_poisoned(k) for k, s in enumerate(arena.slots) if s.role == "out"})
    with pytest.raises(gc.GuardError) as e:
        gc.unwritten("fs_selftest", arena_a.slots, *stills)
    assert (e.value.kind, e.value.arg, e.value.offset) == ("unwritten", 9, 28)
    skip = torch.zeros(40, dtype=torch.bool)
    skip[28:32] = True
    gc.unwritten("fs_selftest", arena_a.slots, *stills, skip={4: skip})     # ... unless documented as left alone


def test_a_kept_region_holds_the_callers_bytes():
    source = torch.arange(16, dtype=torch.uint8)
    keep = torch.zeros(16, dtype=torch.bool)
    keep[4:8] = True
    arena = gc.Arena("cpu", [gc.Slot(0, 16, "out", source, keep)], "A")
    assert arena.view(0).tolist() == [255] * 4 + [4, 5, 6, 7] + [255] * 8


# ---- the interposer, on a stand-in for the library -----------------------------------------------------------------------------
class _FakeLib:
    @staticmethod
    def fs_conv16_work_bytes(batch, dim):
        return 36 * batch


def _interposer(poison, real):
    guard = gc.Interposer(poison, _FakeLib)
    guard.real = real
    return guard


def test_interposer_relocates_checks_and_copies_back():
    seen = {}

    def real(name, device, x, g, batch, dim, dw, work):
        seen["ptrs"] = (x.data_ptr(), g.data_ptr(), dw.data_ptr(), work.data_ptr())
        seen["work"] = work.numel()
        dw.view(torch.float32).copy_(x.view(torch.float32)[:4] + g.view(torch.float32)[:4])
        work.fill_(1)

    x, g = torch.arange(8, dtype=torch.float32), torch.ones(8)
    runs = []
    for poison in gc.POISONS:
        dw, work = torch.empty(4), torch.empty(100, dtype=torch.uint8)
        guard = _interposer(poison, real)
        guard("fs_conv16_wgrad", "cpu", x, g, 2, 64, dw, work)
        assert dw.tolist() == [1.0, 2.0, 3.0, 4.0] and guard.counts == {"fs_conv16_wgrad": 1}
        assert seen["work"] == 72 and all(p % gc.ALIGN == 0 for p in seen["ptrs"])
        assert not {x.data_ptr(), g.data_ptr(), dw.data_ptr(), work.data_ptr()} & set(seen["ptrs"])
        runs.append(guard)
    gc.assert_outputs_written(*runs)


def test_interposer_reports_short_scratch_overruns_and_skipped_elements():
    x, g = torch.arange(8, dtype=torch.float32), torch.ones(8)
    with pytest.raises(gc.GuardError) as e:
        _interposer("A", lambda *a: None)("fs_conv16_wgrad", "cpu", x, g, 2, 64, torch.empty(4), torch.empty(71, dtype=torch.uint8))
    assert (e.value.kind, e.value.entry, e.value.arg) == ("work", "fs_conv16_wgrad", 5)

    def overrun(name, device, x, g, batch, dim, dw, work):   # a torch write one element past the output, through its storage
        past = torch.empty(0, dtype=torch.uint8).set_(dw.untyped_storage(), dw.storage_offset() + dw.numel(), (4,), (1,))
        past.fill_(0)

    with pytest.raises(gc.GuardError) as e:
        _interposer("B", overrun)("fs_conv16_wgrad", "cpu", x, g, 2, 64, torch.empty(4), torch.empty(72, dtype=torch.uint8))
    assert (e.value.kind, e.value.arg, e.value.side, e.value.offset) == ("guard", 4, "after", 0)

    def skips(name, device, x, g, batch, dim, dw, work):
        dw.view(torch.float32)[:3] = 1.0

    runs = []
    for poison in gc.POISONS:
        runs.append(_interposer(poison, skips))
        runs[-1]("fs_conv16_wgrad", "cpu", x, g, 2, 64, torch.empty(4), torch.empty(72, dtype=torch.uint8))
    with pytest.raises(gc.GuardError) as e:
        gc.assert_outputs_written(*runs)
    assert (e.value.kind, e.value.entry, e.value.arg, e.value.offset) == ("unwritten", "fs_conv16_wgrad", 4, 12)


def test_overlapping_arguments_share_a_slot():
    seen = {}

    def real(name, device, x, w, transposed, batch, dim, y):
        seen["x"], seen["y"] = x.data_ptr(), y.data_ptr()
        y.view(torch.float32).copy_(x.view(torch.float32) * 2)

    base = torch.arange(12, dtype=torch.float32)
    x, y = base[:8], base[4:]
    _interposer("A", real)("fs_conv16_forward", "cpu", x, torch.ones(3), 0, 1, 64, y)
    assert seen["y"] - seen["x"] == 16
    assert base.tolist() == [0, 1, 2, 3, 0, 2, 4, 6, 8, 10, 12, 14]
