"""Guard-band buffers: did a kernel stay inside the memory it was given?

`guarded(shape, dtype, device, payload=..., poison=...)` returns a contiguous tensor that is a view into
one flat uint8 allocation laid out as

    [ slack < 256 B | front guard, 1 MiB | payload, numel * itemsize bytes | back guard, 1 MiB ]

The payload starts on a 256-byte boundary (what the caching allocator and the executor's arena give; kernels
may rely on 16), is exactly as long as the tensor, and the back guard starts on the very next byte: no
rounding slack a stray access could hide in.

Guards are filled in one of two ways, and `check()` verifies either bit for bit on the tensor's device:

* ``poison="pattern"`` (write guard; outputs, workspaces, counters, codec frames): the byte 0xA5.
* ``poison="nan"`` / ``"inf"`` (read poison; activations, residuals, packed weights, biases): the dtype's
  NaN or +inf in every guard element, so that a value a kernel reads from outside its tensor and *uses*
  turns the output non-finite.  Both are needed: max-style instructions drop NaN, so a pooling kernel
  shows an over-read only with +inf.  Integer dtypes take an int byte value (``poison=0xFF``).

Known limit: an over-read whose value is discarded (a select on the row / channel mask after the load) is
invisible to this method; only values that reach an output, and every write, are caught.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

GUARD = 1 << 20          # bytes of each guard
ALIGN = 256              # payload alignment
PATTERN = 0xA5           # write-guard byte
NAN, INF = "nan", "inf"

_fills: dict = {}


def _fill_bytes(dtype: torch.dtype, device: torch.device, poison) -> torch.Tensor:
    """GUARD bytes of the guard's content (cached per device / dtype / poison; never written after creation)."""
    if poison == "pattern":
        poison = PATTERN
    key = (str(device), poison if isinstance(poison, int) else (dtype, poison))
    if key not in _fills:
        if isinstance(poison, int):
            unit = torch.tensor([poison], dtype=torch.uint8)
        elif poison in (NAN, INF):
            if not dtype.is_floating_point:
                raise ValueError(f"{poison!r} poison needs a floating dtype, got {dtype}")
            unit = torch.tensor([float(poison)], dtype=dtype).view(torch.uint8)
        else:
            raise ValueError(f"unknown poison {poison!r}")
        _fills[key] = unit.repeat(GUARD // unit.numel()).to(device)
    return _fills[key]


class Guard:
    """Book-keeping of one guarded buffer (reachable as ``guard_of(t)``)."""

    def __init__(self, flat: torch.Tensor, start: int, nbytes: int, fill: torch.Tensor, poison, name: str):
        self.flat, self.start, self.nbytes, self.fill, self.poison, self.name = flat, start, nbytes, fill, poison, name

    @property
    def front(self) -> torch.Tensor:
        return self.flat[self.start - GUARD:self.start]

    @property
    def back(self) -> torch.Tensor:
        return self.flat[self.start + self.nbytes:self.start + self.nbytes + GUARD]

    def damage(self) -> Optional[str]:
        """None if both guards hold their fill bit for bit, else a description of the damage.  Offsets are
        relative to the payload edge: -1 is the byte just before the payload, +0 the byte just after it."""
        msgs = []
        for side, g, base in (("front", self.front, -GUARD), ("back", self.back, 0)):
            if torch.equal(g, self.fill):
                continue
            bad = (g != self.fill).nonzero().flatten()
            first, last = int(bad[0]) + base, int(bad[-1]) + base
            near = last if side == "front" else first
            edge = "start" if side == "front" else "end"
            msgs.append(f"{side} guard damaged: {bad.numel()} bytes, first damaged offset {first:+d} from the "
                        f"payload {edge} (nearest {near:+d}, last {last:+d})")
        return "; ".join(msgs) or None

    def check(self, what: str = "") -> None:
        d = self.damage()
        assert d is None, f"{self.name or 'buffer'}{' ' + what if what else ''} ({self.nbytes} payload bytes): {d}"

    def restore(self) -> None:
        """Put the guards back (after a reported damage, so that later checks of a shared buffer start clean)."""
        self.front.copy_(self.fill)
        self.back.copy_(self.fill)


def guarded(shape, dtype: torch.dtype, device, payload=None, poison="pattern", name: str = "") -> torch.Tensor:
    """A contiguous `shape` / `dtype` tensor on `device` between two 1 MiB guards (module docstring).
    `payload`: None (left as allocated), a scalar to fill with, or a tensor / array to copy in."""
    device = torch.device(device)
    shape = (shape,) if isinstance(shape, int) else tuple(int(s) for s in shape)
    itemsize = torch.empty((), dtype=dtype).element_size()
    nbytes = math.prod(shape) * itemsize
    flat = torch.empty(ALIGN - 1 + GUARD + nbytes + GUARD, dtype=torch.uint8, device=device)
    start = GUARD + (-(flat.data_ptr() + GUARD)) % ALIGN
    fill = _fill_bytes(dtype, device, poison)
    g = Guard(flat, start, nbytes, fill, poison, name)
    g.restore()
    t = flat[start:start + nbytes].view(dtype).view(shape)
    if payload is not None:
        if isinstance(payload, (int, float)):
            t.fill_(payload)
        else:
            if isinstance(payload, np.ndarray):
                payload = torch.from_numpy(np.array(payload))        # a writable copy
            t.copy_(payload.reshape(shape))
    t._guardband = g
    return t


def rehome(t: torch.Tensor, poison="pattern", name: str = "") -> torch.Tensor:
    """A guarded copy of `t` (same shape, dtype, device, contents): ``pc.w = rehome(pc.w, poison=NAN)``."""
    return guarded(t.shape, t.dtype, t.device, payload=t, poison=poison, name=name)


def guard_of(t: torch.Tensor) -> Guard:
    return t._guardband


def check(*tensors, what: str = "") -> None:
    """Assert that the guards of every given tensor (None entries are skipped) are intact."""
    for t in tensors:
        if t is not None:
            guard_of(t).check(what)
