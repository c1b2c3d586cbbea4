"""Guard-band runs of the GPU codecs (lz4_gpu.hip, zvc_gpu.hip, zfp_gpu.hip; tests/guardband.py).

Each codec's `frame` / `out`, `scratch`, `sizes`, `offs` and `total` are re-homed into guarded buffers of
exactly the size its constructor computed (`lz4_gpu_max_frame`, `lz4_gpu_scratch_bytes`, `zvc_max_stream`,
`zvc_scratch_bytes`, `zfp_gpu_maxw` words per block); the codecs read `data_ptr()` at call time.  Inputs stress the
bound, not the ratio: incompressible random bits, all zeros, and a post-ReLU-like half-zero tensor, at lengths
around every chunk / segment / block boundary and at the codec's capacity.  Asserted: every guard intact, the
reported size within the promised bound, the GPU round trip bit-exact (decoded from a guarded device copy of the
frame whose guards hold 0xFF bytes -- NaN in every float format -- into a guarded output), and for LZ4 and ZVC
the frame also decodes bit-exactly through the host codec.  GpuZFP.decompress takes host bytes and stages its
own device copy, so only its output and tables are guarded on the way back.
"""
import importlib

import numpy as np
import pytest
import torch

import guardband as G

PKG = "adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd"

pytestmark = pytest.mark.gpu

KINDS = ("random", "zeros", "relu")
U8 = torch.uint8


def _bytes(nbytes, kind, seed):
    """`nbytes` of test data as a CPU uint8 tensor."""
    g = torch.Generator().manual_seed(seed)
    if kind == "random":
        return torch.randint(0, 256, (nbytes,), dtype=U8, generator=g)
    if kind == "zeros":
        return torch.zeros(nbytes, dtype=U8)
    v = torch.relu(torch.randn((nbytes + 1) // 2, generator=g)).to(torch.bfloat16)      # ~half exact zeros
    return v.view(U8)[:nbytes].clone()


def _rehome_attrs(codec, names):
    for nm in names:
        setattr(codec, nm, G.rehome(getattr(codec, nm), name=f"{type(codec).__name__}.{nm}"))
    return [getattr(codec, nm) for nm in names]


def _dev_in(raw, dtype=U8):
    t = G.guarded(raw.numel(), U8, "cuda", payload=raw, poison=0xFF, name="input")
    return t if dtype == U8 else _typed(t, dtype)


def _typed(t, dtype):
    v = t.view(dtype)
    v._guardband = G.guard_of(t)
    return v


@pytest.mark.parametrize("kind", KINDS)
def test_guard_gpu_lz4(kind):
    gl = importlib.import_module(f"{PKG}.codec.gpu_lz4")
    rt = importlib.import_module(f"{PKG}.native").runtime()
    K = importlib.import_module(f"{PKG}.ops._lib").kernels()
    chunk = K.lz4_gpu_chunk()
    max_bytes = 5 * chunk + 333
    codec = gl.GpuLZ4(max_bytes)
    assert codec.frame.numel() == K.lz4_gpu_max_frame(max_bytes)
    assert codec.scratch.numel() == max(1, K.lz4_gpu_scratch_bytes(max_bytes))
    assert codec.sizes.numel() == codec.offs.numel() == -(-max_bytes // chunk)
    bufs = _rehome_attrs(codec, ("frame", "scratch", "sizes", "offs", "total", "err"))
    for n in (1, chunk - 1, chunk, chunk + 1, 3 * chunk + 17, max_bytes):
        raw = _bytes(n, kind, n)
        x = _dev_in(raw)
        codec.compress(x)
        frame = codec.frame_bytes()
        torch.cuda.synchronize()
        G.check(x, *bufs, what=f"[lz4 compress {kind} {n} B]")
        assert len(frame) == int(codec.total.item()) <= K.lz4_gpu_max_frame(n) <= codec.frame.numel()
        assert rt.lz4_decompress(frame) == raw.numpy().tobytes(), f"host decode, {kind} {n} B"
        dframe = G.guarded(len(frame), U8, "cuda", payload=np.frombuffer(frame, np.uint8), poison=0xFF,
                           name="device frame")
        out = G.guarded(n, U8, "cuda", payload=0xEE, name="decoded")
        codec.decompress(dframe, out)
        torch.cuda.synchronize()
        G.check(dframe, out, *bufs, what=f"[lz4 decompress {kind} {n} B]")
        assert torch.equal(out.cpu(), raw), f"GPU round trip, {kind} {n} B"


@pytest.mark.parametrize("esz,dtype", [(2, torch.bfloat16), (4, torch.float32)])
@pytest.mark.parametrize("kind", KINDS)
def test_guard_gpu_zvc(kind, esz, dtype):
    gz = importlib.import_module(f"{PKG}.codec.gpu_zvc")
    rt = importlib.import_module(f"{PKG}.native").runtime()
    K = importlib.import_module(f"{PKG}.ops._lib").kernels()
    seg = K.zvc_seg()
    max_elems = 5 * seg + 77
    codec = gz.GpuZVC(max_elems, esz)
    assert codec.out.numel() == K.zvc_max_stream(max_elems, esz)
    assert codec.scratch.numel() == K.zvc_scratch_bytes(max_elems, esz)
    assert codec.sizes.numel() == codec.offs.numel() == -(-max_elems // seg)
    bufs = _rehome_attrs(codec, ("out", "scratch", "sizes", "offs", "total"))
    for n in (1, 63, 64, 65, seg - 1, seg, seg + 1, 3 * seg + 17, max_elems):
        raw = _bytes(n * esz, kind, n + esz)
        x = _dev_in(raw, dtype)
        codec.compress(x)
        s = codec.stream_bytes()
        torch.cuda.synchronize()
        G.check(x, *bufs, what=f"[zvc compress {kind} {n} x {esz} B]")
        assert len(s) == int(codec.total.item()) <= K.zvc_max_stream(n, esz) <= codec.out.numel()
        assert s == rt.zvc_compress(raw.numpy(), esz), f"host encoder bytes, {kind} {n}"
        assert rt.zvc_decompress(s) == raw.numpy().tobytes(), f"host decode, {kind} {n}"
        dstream = G.guarded(len(s), U8, "cuda", payload=np.frombuffer(s, np.uint8), poison=0xFF, name="device stream")
        out = _typed(G.guarded(n * esz, U8, "cuda", payload=0xEE, name="decoded"), dtype)
        codec.decompress(dstream, out)
        torch.cuda.synchronize()
        G.check(dstream, out, *bufs, what=f"[zvc decompress {kind} {n} x {esz} B]")
        assert torch.equal(out.view(U8).cpu(), raw), f"GPU round trip, {kind} {n}"


# whole blocks, one element past a block edge in one / every axis, prime extents (every fold pads)
ZFP_SHAPES = [(1,), (4,), (5,), (13,), (4, 4), (5, 4), (7, 5), (4, 4, 4), (3, 5, 7), (5, 9, 13), (2, 3, 5, 7),
              (3, 7, 7, 36)]


@pytest.mark.parametrize("shape", ZFP_SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_guard_gpu_zfp(kind, shape):
    from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.codec import zfp_shape
    gzf = importlib.import_module(f"{PKG}.codec.gpu_zfp")
    rt = importlib.import_module(f"{PKG}.native").runtime()
    K = importlib.import_module(f"{PKG}.ops._lib").kernels()
    z = gzf.GpuZFP(shape)
    maxw = int(K.zfp_gpu_maxw(len(z.zshape)))
    assert z.scratch.numel() == z.nblocks * maxw and z.out.numel() == z.nblocks * (1 + maxw)
    assert z.offs.numel() == z.nblocks
    bufs = _rehome_attrs(z, ("out", "scratch", "offs", "total"))
    n = int(np.prod(shape))
    raw = _bytes(4 * n, "random" if kind == "random" else "zeros", n)
    if kind == "relu":
        raw = torch.relu(torch.randn(n, generator=torch.Generator().manual_seed(n))).view(U8).clone()
    xin =G.guarded(shape, torch.float32, "cuda", payload=raw.view(torch.float32).reshape(shape), poison=G.NAN,
                    name="input")
    z.compress(xin)
    c = z.container()
    torch.cuda.synchronize()
    G.check(xin, *bufs, what=f"[zfp compress {kind} {shape}]")
    words = int(z.total.item())
    assert z.nblocks + words <= z.out.numel() and words <= z.nblocks * maxw
    host = rt.zfp_compress(raw.view(torch.float32).numpy().reshape(zfp_shape(shape)), 4, 1)
    assert c == host, f"host encoder bytes, {kind} {shape}"
    out = G.guarded(shape, torch.float32, "cuda", payload=float("nan"), name="decoded")
    z.decompress(c, out)
    torch.cuda.synchronize()
    G.check(out, *bufs, what=f"[zfp decompress {kind} {shape}]")
    assert torch.equal(out.view(U8).cpu().reshape(-1), raw), f"GPU round trip, {kind} {shape}"
