"""The guard-band helper itself (tests/guardband.py): layout, fills, and that a one-byte write just outside
the payload, made with plain torch indexing into the test's own flat buffer, is reported with its offset."""
import re

import numpy as np
import pytest
import torch

import guardband as G

CASES = [((3, 5, 7), torch.float32), ((1,), torch.uint8), ((129,), torch.bfloat16), ((2, 3), torch.int32),
         ((5, 3), torch.float64)]


@pytest.mark.parametrize("shape,dtype", CASES)
def test_layout(shape, dtype):
    t = G.guarded(shape, dtype, "cpu", payload=0)
    g = G.guard_of(t)
    assert t.is_contiguous() and tuple(t.shape) == shape and t.dtype == dtype
    assert t.data_ptr() % G.ALIGN == 0
    assert g.nbytes == t.numel() * t.element_size()
    assert t.data_ptr() == g.flat.data_ptr() + g.start
    # the guards touch the payload on both sides, each exactly 1 MiB, all inside the one allocation
    assert g.front.numel() == G.GUARD and g.back.numel() == G.GUARD
    assert g.front.data_ptr() + G.GUARD == t.data_ptr()
    assert g.back.data_ptr() == t.data_ptr() + g.nbytes
    assert g.back.data_ptr() + G.GUARD <= g.flat.data_ptr() + g.flat.numel()
    assert g.start - G.GUARD >= 0
    G.check(t)


def test_fills():
    t = G.guarded((4, 3), torch.float32, "cpu", payload=1.5)
    g = G.guard_of(t)
    assert bool((g.front == G.PATTERN).all()) and bool((g.back == G.PATTERN).all())
    assert bool((t == 1.5).all())
    t = G.guarded((7,), torch.float32, "cpu", poison=G.NAN)
    g = G.guard_of(t)
    assert bool(torch.isnan(g.back.view(torch.float32)).all()) and bool(torch.isnan(g.front.view(torch.float32)).all())
    # the element straight after / before the payload is a whole poison value (the phase matches the payload's)
    whole = g.flat[g.start - 4:g.start + g.nbytes + 4].view(torch.float32)
    assert bool(torch.isnan(whole[0])) and bool(torch.isnan(whole[-1]))
    t = G.guarded((7,), torch.bfloat16, "cpu", poison=G.INF)
    g = G.guard_of(t)
    assert bool((g.back.view(torch.bfloat16) == float("inf")).all())
    assert bool((g.front.view(torch.bfloat16) == float("inf")).all())
    t = G.guarded((5,), torch.uint8, "cpu", poison=0xFF)
    assert bool((G.guard_of(t).back == 0xFF).all())
    with pytest.raises(ValueError):
        G.guarded((5,), torch.int32, "cpu", poison=G.NAN)
    G.check(t, None)


def test_rehome_keeps_contents():
    src = torch.arange(35, dtype=torch.float32).reshape(5, 7)
    t = G.rehome(src, poison=G.NAN)
    assert torch.equal(t, src) and t.data_ptr() != src.data_ptr() and t.data_ptr() % G.ALIGN == 0
    t2 = G.guarded((5, 7), torch.float32, "cpu", payload=src.numpy())
    assert torch.equal(t2, src)
    G.check(t, t2)


def _offsets(msg):
    return [int(m) for m in re.findall(r"first damaged offset ([+-]\d+)", msg)]


@pytest.mark.parametrize("poison", ["pattern", G.NAN, G.INF])
@pytest.mark.parametrize("where,offset", [("before", -1), ("after", 0), ("before", -G.GUARD), ("after", G.GUARD - 1),
                                          ("after", 4096)])
def test_one_byte_write_is_reported_with_its_offset(poison, where, offset):
    t = G.guarded((3, 11), torch.float32, "cpu", payload=float("nan"), poison=poison, name="victim")
    g = G.guard_of(t)
    edge = g.start if where == "before" else g.start + g.nbytes
    g.flat[edge + offset] ^= 0x01
    with pytest.raises(AssertionError) as e:
        G.check(t, what="after the write")
    msg = str(e.value)
    assert "victim" in msg and ("front" if where == "before" else "back") in msg
    assert _offsets(msg) == [offset], msg
    assert "1 bytes" in msg
    g.restore()
    G.check(t)


def test_both_sides_and_payload_writes():
    t = G.guarded((16,), torch.int32, "cpu", payload=0)
    g = G.guard_of(t)
    t.fill_(-1)                                  # writes inside the payload never trip a guard
    g.flat[g.start:g.start + g.nbytes] = 0x5A
    G.check(t)
    g.flat[g.start - 3] = 0
    g.flat[g.start + g.nbytes + 7] = 0
    g.flat[g.start + g.nbytes + 9] = 0
    d = g.damage()
    assert _offsets(d) == [-3, 7] and "2 bytes" in d and "last +9" in d


@pytest.mark.gpu
@pytest.mark.parametrize("offset", [-1, 0])
def test_one_byte_write_on_the_device(offset):
    t = G.guarded((5, 3, 64), torch.float32, "cuda", payload=float("nan"), poison=G.NAN)
    g = G.guard_of(t)
    assert t.is_cuda and t.data_ptr() % G.ALIGN == 0 and g.flat.is_cuda
    G.check(t)
    edge = g.start if offset < 0 else g.start + g.nbytes
    g.flat[edge + offset] ^= 0x01                # (a plain 0 would be a no-op on the NaN's low byte)
    with pytest.raises(AssertionError) as e:
        G.check(t)
    assert _offsets(str(e.value)) == [offset] and "1 bytes" in str(e.value)
    assert bool(torch.isnan(t).all())            # the payload itself was not touched
    assert np.isnan(t.cpu().numpy()).all()
