"""CPU side of select / resample on a rollout session (sea_amd/rollout_session.py): the index check is a pure function, sea_kv_cache_gather is exported,
refuses every malformed table on the host and reads SeaKvGather with the layout of the binding, ops.kv_cache_gather validates its index before any
operand's address is taken, and the pointer audit states the extents of all four layout combinations."""
import ctypes as C
import re

import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from sea_amd import build, _native

    build.build(verbose=False)
    return _native.lib()


# ------------------------------------------------------------------------------------------------ check_select
def test_check_select_accepts_lists_tuples_and_integer_tensors():
    from sea_amd.rollout_session import check_select

    assert check_select(3, [2, 0, 0, 2, 2]) == [2, 0, 0, 2, 2]
    assert check_select(3, (1,)) == [1]
    assert check_select(4, torch.tensor([3, 0, 3], dtype=torch.int32)) == [3, 0, 3]
    assert check_select(4, torch.tensor([1, 2], dtype=torch.int64)) == [1, 2]
    out = check_select(66, [i % 2 for i in range(66)])
    assert len(out) == 66 and all(type(v) is int for v in out)


@pytest.mark.parametrize("index,what", [
    ([], "empty"), ((), "empty"), (torch.zeros(0, dtype=torch.int64), "empty"),
    ([[0, 1]], "1-D"), (torch.zeros(2, 2, dtype=torch.int64), "1-D"), (torch.tensor(1), "1-D"),
    ([0.0, 1.0], "integers"), ([True, False], "integers"), (torch.tensor([0.0, 1.0]), "integer tensor"), (torch.tensor([True, False]), "integer tensor"),
    (torch.tensor([0, 1], dtype=torch.bfloat16), "integer tensor"),
    ([0, 3], r"\[0, B_src = 3\)"), ([-1, 0], r"\[0, B_src = 3\)"), (torch.tensor([0, 1, 7]), r"\[0, B_src = 3\)"), (torch.tensor([-2], dtype=torch.int32), r"\[0, B_src = 3\)"),
    (5, "list, a tuple or an integer tensor"), ("012", "list, a tuple or an integer tensor"),
])
def test_check_select_rejects_malformed_indices(index, what):
    from sea_amd.rollout_session import check_select

    with pytest.raises(ValueError, match=what):
        check_select(3, index)


# ------------------------------------------------------------------------------------------------ the entry point on the host
def test_gather_symbol_and_struct(lib):
    from sea_amd import _native as N

    assert hasattr(lib, "sea_kv_cache_gather") and "sea_kv_cache_gather" in N.EXPORTED_SYMBOLS
    assert N.KV_GATHER_MAX == 32 and lib.sea_abi_version() == 8
    assert C.sizeof(N.SeaKvGather) == 64
    assert [f[0] for f in N.SeaKvGather._fields_] == ["src", "dst", "index", "B_src", "B_dst", "H", "hd", "n_pos", "cap_src", "cap_dst", "src_transposed",
                                                      "dst_transposed", "pad_"]


def _entry(e, **over):
    e.src, e.dst, e.index = 0x10000, 0x80000, 0x4000       # never dereferenced: every call below is refused on the host
    e.B_src, e.B_dst, e.H, e.hd, e.n_pos, e.cap_src, e.cap_dst, e.src_transposed, e.dst_transposed = 2, 5, 3, 16, 5, 8, 16, 0, 1
    for k, v in over.items():
        setattr(e, k, v)


def test_gather_refusals_without_gpu(lib):
    from sea_amd import _native as N

    arr = (N.SeaKvGather * 2)()
    name = b"sea_kv_cache_gather"
    assert lib.sea_kv_cache_gather(None, 1, N.SEA_BF16, None) == -1 and name + b": bad arguments" in lib.sea_last_error()
    _entry(arr[0])
    assert lib.sea_kv_cache_gather(arr, 0, N.SEA_BF16, None) == -1 and name + b": bad arguments" in lib.sea_last_error()      # n = 0
    assert lib.sea_kv_cache_gather(arr, 1, 7, None) == -1 and name + b": bad dtype 7" in lib.sea_last_error()
    for over in (dict(src=None), dict(dst=None), dict(index=None), dict(src=0x10004), dict(dst=0x80008)):
        _entry(arr[0], **over)
        assert lib.sea_kv_cache_gather(arr, 1, N.SEA_F32, None) == -1 and name + b": entry 0: null or misaligned" in lib.sea_last_error(), over
    for over in (dict(hd=12), dict(hd=0), dict(hd=264), dict(n_pos=17, cap_src=24), dict(n_pos=9), dict(n_pos=0), dict(cap_src=12), dict(cap_dst=20),
                 dict(src_transposed=2), dict(dst_transposed=2), dict(dst_transposed=-1), dict(B_src=0), dict(B_dst=0), dict(H=0)):
        _entry(arr[0], **over)
        assert lib.sea_kv_cache_gather(arr, 1, N.SEA_BF16, None) == -1, over
        assert name + b": entry 0: bad sizes" in lib.sea_last_error(), over
    # source and destination may not share a byte: src is 2 * 3 * 8 * 16 bf16 = 1536 bytes
    for dst in (0x10000, 0x10000 + 1520, 0x10000 - 16):
        _entry(arr[0], dst=dst)
        assert lib.sea_kv_cache_gather(arr, 1, N.SEA_BF16, None) == -1 and name + b": entry 0: source and destination overlap" in lib.sea_last_error(), hex(dst)
    # the message names the entry that is wrong
    _entry(arr[0])
    _entry(arr[1], index=None)
    assert lib.sea_kv_cache_gather(arr, 2, N.SEA_F32, None) == -1 and name + b": entry 1: null" in lib.sea_last_error()
    # more workgroups than a launch grid holds (src and dst far apart: 2^53 bytes each)
    _entry(arr[0], dst=1 << 56, B_src=1 << 20, B_dst=1 << 20, H=1 << 10, hd=256, n_pos=8192, cap_src=8192, cap_dst=8192)
    assert lib.sea_kv_cache_gather(arr, 1, N.SEA_F32, None) == -1 and name + b": " in lib.sea_last_error() and b"workgroups" in lib.sea_last_error()


def test_library_reads_the_struct_with_the_bindings_layout(lib):
    """SeaKvGather is not in sea_struct_sizes' table (that one keeps SeaKvFork last), so its layout is held against the library directly: a refusal
    prints every integer field, and the second element of an array is found where the binding puts it."""
    from sea_amd import _native as N

    arr = (N.SeaKvGather * 2)()
    vals = dict(B_src=11, B_dst=12, H=13, hd=12, n_pos=15, cap_src=16, cap_dst=24, src_transposed=1, dst_transposed=0)
    _entry(arr[0])
    _entry(arr[1], **vals)
    assert lib.sea_kv_cache_gather(arr, 2, N.SEA_F32, None) == -1
    msg = lib.sea_last_error().decode()
    assert "entry 1: bad sizes" in msg
    assert {k: int(v) for k, v in re.findall(r"(\w+)=(-?\d+)", msg)} == vals


# ------------------------------------------------------------------------------------------------ ops.kv_cache_gather
def test_kv_cache_gather_checks_the_index_before_any_device_call(monkeypatch):
    from sea_amd import _native as N, ops

    monkeypatch.setattr(N, "lib", lambda: pytest.fail("the library was reached"))
    monkeypatch.setattr(N, "require_gpu", lambda *a, **k: pytest.fail("the operands were looked at"))
    monkeypatch.setattr(torch.Tensor, "data_ptr", lambda self: pytest.fail("an address was taken"))
    src, dst = torch.zeros(3, 2, 8, 8), torch.zeros(4, 2, 8, 8)
    e = [dict(src=src, dst=dst, n_pos=4, src_transposed=False, dst_transposed=False)]
    for index, what in (([0, 1, 2, 3], r"\[0, B_src = 3\)"), ([0, -1, 2, 1], r"\[0, B_src = 3\)"), (torch.tensor([0, 1, 5, 1]), r"\[0, B_src = 3\)"),
                        ([0, 1, 2], "B_dst = 4"), ([0, 1, 2, 0, 1], "B_dst = 4"), ([], "empty"), (torch.zeros(2, 2, dtype=torch.int64), "1-D"),
                        ([0.0, 1.0, 2.0, 0.0], "integers"), (torch.tensor([0.0, 1.0, 2.0, 0.0]), "integer tensor")):
        with pytest.raises(ValueError, match=what):
            ops.kv_cache_gather(e, index, torch.float32)
    # the smallest B_src of several entries bounds the index
    e2 = e + [dict(src=torch.zeros(2, 2, 8, 8), dst=dst, n_pos=4, src_transposed=False, dst_transposed=False)]
    with pytest.raises(ValueError, match=r"\[0, B_src = 2\)"):
        ops.kv_cache_gather(e2, [0, 1, 2, 0], torch.float32)


def test_kv_cache_gather_refuses_cpu_operands_after_a_good_index():
    from sea_amd import ops

    e = [dict(src=torch.zeros(3, 2, 8, 8), dst=torch.zeros(4, 2, 8, 8), n_pos=4, src_transposed=False, dst_transposed=False)]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.kv_cache_gather(e, [0, 2, 2, 1], torch.float32)


# ------------------------------------------------------------------------------------------------ the pointer audit
def _extents(g, esz):
    from sea_amd import ptrcheck

    return {name: (p, n) for name, p, n in ptrcheck._extents(g, esz)}


def _slab_end(B, H, hd, cap, n_pos, transposed):
    """Elements from the start of a cache tensor to one past the last element of positions < n_pos, counted element by element over the last (b, h)."""
    last = 0
    for p in (0, n_pos - 1):
        for d in (0, hd - 1):
            off = d * cap + p if transposed else p * hd + d
            last = max(last, off)
    return (B * H - 1) * cap * hd + last + 1


@pytest.mark.parametrize("esz", [2, 4])
@pytest.mark.parametrize("src_t,dst_t", [(0, 0), (1, 1), (0, 1), (1, 0)])
def test_ptrcheck_extents_of_a_gather(src_t, dst_t, esz):
    from sea_amd import _native as N

    g = N.SeaKvGather()
    g.src, g.dst, g.index = 0x7000_0000_0000, 0x7100_0000_0000, 0x7200_0000_0000
    g.B_src, g.B_dst, g.H, g.hd, g.n_pos, g.cap_src, g.cap_dst, g.src_transposed, g.dst_transposed = 3, 5, 2, 48, 13, 16, 40, src_t, dst_t
    ext = _extents(g, esz)
    assert set(ext) == {"src", "dst", "index"}
    assert ext["src"] == (g.src, _slab_end(3, 2, 48, 16, 13, src_t) * esz)
    assert ext["dst"] == (g.dst, _slab_end(5, 2, 48, 40, 13, dst_t) * esz)
    assert ext["index"] == (g.index, 5 * 4)
    g.cap_dst = 64
    assert _extents(g, esz)["dst"][1] == _slab_end(5, 2, 48, 64, 13, dst_t) * esz > ext["dst"][1]
    assert _extents(g, esz)["src"] == ext["src"]
    g.cap_dst, g.B_dst = 40, 9
    grown = _extents(g, esz)
    assert grown["dst"][1] == _slab_end(9, 2, 48, 40, 13, dst_t) * esz == ext["dst"][1] + 4 * 2 * 40 * 48 * esz
    assert grown["index"][1] == 9 * 4 and grown["src"] == ext["src"]


def test_ptrcheck_refuses_a_gather_that_leaves_its_buffers():
    """check_records over a hand-made record: every pointer must lie in a known range and every extent must end inside it."""
    from types import SimpleNamespace

    from sea_amd import _native as N, ptrcheck

    arr = (N.SeaKvGather * 1)()
    g = arr[0]
    g.src, g.dst, g.index = 0x7000_0000_0000, 0x7100_0000_0000, 0x7200_0000_0000
    g.B_src, g.B_dst, g.H, g.hd, g.n_pos, g.cap_src, g.cap_dst, g.src_transposed, g.dst_transposed = 3, 5, 2, 8, 13, 16, 24, 0, 1
    R = ptrcheck.Ranges()
    R.add_range(g.src, 3 * 2 * 16 * 8 * 4, "src")
    R.add_range(g.dst, 5 * 2 * 24 * 8 * 4, "dst")
    R.add_range(g.index, 5 * 4, "index")
    rec = SimpleNamespace(fn=object(), args=[arr, 1, 0], keep=arr, name="kv.cache_gather")
    assert ptrcheck.check_records([rec], R, 4, "test") > 0
    g.B_dst = 6
    with pytest.raises(RuntimeError, match=r"SeaKvGather\.dst .*past the end of its buffer"):
        ptrcheck.check_records([rec], R, 4, "test")
    g.B_dst, g.B_src = 5, 4
    with pytest.raises(RuntimeError, match=r"SeaKvGather\.src .*past the end of its buffer"):
        ptrcheck.check_records([rec], R, 4, "test")
    g.B_src = 3
    g.index += 1 << 30
    with pytest.raises(RuntimeError, match=r"SeaKvGather\.index = .* lies in no buffer"):
        ptrcheck.check_records([rec], R, 4, "test")
