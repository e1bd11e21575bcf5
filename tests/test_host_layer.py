"""The host layer under every handle, decided on the CPU: how a handle owns device memory (WgDevMem), checks a caller's pointer
(wg_on_device) and frames its state blob (wg_blob_get / wg_blob_set) is windgym_amd/csrc/wg_host.h, which names HIP but includes
none of it.  tests/host_layer_shim.cpp puts a scripted fake device in front of the header, so the paths a failing HIP call takes —
which no shared GPU can be asked to walk — are walked here.  The Python side (binding.Handle, binding.tensor_ptr) runs on a stub
library and on CPU tensors."""
import ctypes as C
import os
import subprocess

import pytest

from helpers import host_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "windgym_amd", "csrc")
MALLOC, MEMSET, SETDEVICE = 0, 1, 2                     # the shim's fake::Op
SYNC, FREE, COPY = 1, 2, 3                              # the shim's fake::Event
OOM, INVALID_VALUE, INVALID_DEVICE = 2, 1, 101          # the stand-ins' error codes and what hipGetErrorString says to them
ERR_TEXT = {OOM: "out of memory", INVALID_VALUE: "invalid argument", INVALID_DEVICE: "invalid device ordinal"}
HOST, DEVICE = 1, 2                                     # the stand-ins' memory types


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    """g++ alone, no ROCm include path: the header must stay free of HIP headers."""
    lib = host_shim(tmp_path_factory, "host_layer")
    lib.last_error.restype = C.c_char_p
    lib.fake_foreign.restype = C.c_void_p
    lib.fake_frees_of.argtypes = [C.c_void_p]
    lib.fake_malloc_bytes.restype = C.c_size_t
    lib.fake_events.argtypes = [C.POINTER(C.c_int), C.c_int]
    lib.owner_new.restype = C.c_void_p
    lib.owner_delete.argtypes = lib.owner_release.argtypes = lib.owner_held.argtypes = [C.c_void_p]
    lib.owner_alloc.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_int, C.POINTER(C.c_void_p)]
    lib.owner_free.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p]
    lib.on_device.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_char_p, C.c_char_p]
    lib.on_device_all.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.c_char_p]
    lib.blob_header_bytes.restype = C.c_size_t
    lib.blob_magic.restype = C.c_uint32
    lib.blob_get.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.POINTER(C.c_size_t), C.c_size_t]
    lib.blob_set.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_size_t, C.c_char_p, C.c_int, C.c_int]
    lib.INVALID, lib.HIP, lib.NOMEM = lib.err_codes(0), lib.err_codes(1), lib.err_codes(2)
    return lib


def events(shim):
    buf = (C.c_int * 64)()
    return list(buf[:shim.fake_events(buf, 64)])


def last(shim):
    return shim.last_error().decode()


class Owner:
    """A WgDevMem on device 1 while device 0 is current, and the pointers its allocations returned."""

    def __init__(self, shim, device=1):
        shim.fake_reset()
        self.shim, self.m, self.ptrs = shim, shim.owner_new(device), []

    def alloc(self, n=8, zero=True):
        p = C.c_void_p()
        rc = self.shim.owner_alloc(self.m, b"who_create", n, int(zero), C.byref(p))
        if rc == 0:
            self.ptrs.append(p.value)
        return rc

    def build(self, n_allocs=5):
        """-> the rc of the first allocation that failed (0: none did), as a create's chain stops there"""
        for _ in range(n_allocs):
            rc = self.alloc()
            if rc:
                return rc
        return 0

    def release(self):
        self.shim.owner_release(self.m)

    def __del__(self):
        self.shim.owner_delete(self.m)


# ---- the owner ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", [MALLOC, MEMSET])
@pytest.mark.parametrize("err", [OOM, INVALID_VALUE])
@pytest.mark.parametrize("k", range(5))
def test_owner_failing_allocation(shim, k, err, op):
    o = Owner(shim)
    shim.fake_fail(op, k, err)
    rc = o.build()
    assert rc == (shim.NOMEM if err == OOM else shim.HIP)
    assert last(shim) == "who_create: " + ERR_TEXT[err]
    # everything allocated before is still the owner's, and nothing else is: the allocation whose memset failed was given back
    assert shim.fake_n_live() == k and shim.owner_held(o.m) == k and len(o.ptrs) == k
    assert shim.fake_n_frees() == (1 if op == MEMSET else 0)
    # the handle's ordinary destroy
    o.release()
    assert shim.fake_n_live() == 0 and shim.owner_held(o.m) == 0
    assert all(shim.fake_frees_of(p) == 1 for p in o.ptrs) and shim.fake_most_frees() <= 1


def test_owner_allocates_on_its_device(shim):
    o = Owner(shim)
    assert shim.fake_current() == 0
    assert o.build() == 0
    assert shim.fake_current() == 1 and shim.fake_n_live() == 5
    assert all(shim.on_device(b"", 1, p, b"p", b"") == 0 for p in o.ptrs)


def test_owner_release(shim):
    o = Owner(shim)
    assert o.build() == 0
    shim.fake_set_current(0)
    o.release()
    assert events(shim) == [SYNC] + [FREE] * 5            # one synchronise, then the frees ...
    assert shim.fake_n_sync() == 1 and shim.fake_sync_device(0) == 1      # ... with the owner's device current
    assert shim.fake_n_live() == 0 and all(shim.fake_frees_of(p) == 1 for p in o.ptrs)
    o.release()                                           # the owner is empty: nothing more happens
    assert events(shim) == [SYNC] + [FREE] * 5 and shim.fake_n_sync() == 1


def test_owner_release_with_no_allocation_touches_nothing(shim):
    o = Owner(shim)
    o.release()
    assert events(shim) == [] and shim.fake_current() == 0


def test_owner_release_when_the_device_cannot_be_made_current(shim):
    """wg_host.h's rule: the synchronisation is skipped, every pointer is freed all the same."""
    o = Owner(shim)
    assert o.build() == 0
    shim.fake_set_current(0)
    shim.fake_fail(SETDEVICE, 1, INVALID_DEVICE)          # (call 0 was the first allocation's)
    o.release()
    assert events(shim) == [FREE] * 5 and shim.fake_n_sync() == 0
    assert shim.fake_n_live() == 0 and shim.fake_most_frees() == 1 and shim.owner_held(o.m) == 0


def test_owner_alloc_when_the_device_cannot_be_made_current(shim):
    o = Owner(shim)
    shim.fake_fail(SETDEVICE, 0, INVALID_DEVICE)
    assert o.alloc() == shim.HIP
    assert last(shim) == "hipSetDevice: invalid device ordinal"
    assert shim.fake_n_live() == 0 and shim.owner_held(o.m) == 0


def test_owner_free_of_one_pointer(shim):
    o = Owner(shim)
    assert o.build() == 0
    assert shim.owner_free(o.m, b"who_regrow", o.ptrs[2]) == 0
    assert shim.fake_frees_of(o.ptrs[2]) == 1 and shim.fake_n_live() == 4 and shim.owner_held(o.m) == 4
    assert shim.owner_free(o.m, b"who_regrow", o.ptrs[2]) == 0          # no longer the owner's: nothing happens
    assert shim.owner_free(o.m, b"who_regrow", None) == 0
    assert shim.fake_n_frees() == 1
    o.release()
    assert shim.fake_n_live() == 0 and shim.fake_most_frees() == 1 and shim.fake_n_frees() == 5


def test_owner_alloc_of_nothing_is_one_element(shim):
    o = Owner(shim)
    assert o.alloc(n=0) == 0 and o.alloc(n=3) == 0
    assert shim.fake_malloc_bytes(0) == 4 and shim.fake_malloc_bytes(1) == 12          # (the shim allocates floats)


# ---- the pointer check -------------------------------------------------------------------------------------------------------------
# (who opens the null form, prefix the two others, whose closes the wrong-device form): the four families a caller can see
FAMILIES = {
    "curriculum": (b"wg_curriculum_shape: ", b"wg_curriculum: ", b", the device of the handle the curriculum was created on"),
    "expert_labels": (b"wg_expert_labels: ", b"wg_expert_labels: ", b", the handle's device"),
    "yaw_table": (b"wg_yaw_table_rows: ", b"wg_yaw_table_rows: ", b", the table's device"),
    "ppo": (b"wg_ppo_apply: ", b"wg_ppo_apply: ", b""),
}


def table(shim, family, ptrs, required):
    who, prefix, whose = FAMILIES[family]
    names = [b"first_dev", b"second_dev", b"third_out"]
    return shim.on_device_all(who, prefix, 1, (C.c_void_p * 3)(*ptrs), (C.c_char_p * 3)(*names), (C.c_int * 3)(*map(int, required)), whose)


@pytest.mark.parametrize("family", FAMILIES)
def test_pointer_check(shim, family):
    who, prefix, whose = (s.decode() for s in FAMILIES[family])
    shim.fake_reset()
    good, other = shim.fake_foreign(1, DEVICE), shim.fake_foreign(1, DEVICE)
    host, dev0, unknown = shim.fake_foreign(1, HOST), shim.fake_foreign(0, DEVICE), 0x7f0000001000
    one = lambda p: shim.on_device(prefix.encode(), 1, p, b"x_dev", whose.encode())      # noqa: E731
    assert one(good) == 0
    assert one(unknown) == shim.INVALID and last(shim) == f"{prefix}x_dev is not a device pointer"
    assert one(host) == shim.INVALID and last(shim) == f"{prefix}x_dev is not memory of device 1{whose}"
    assert one(dev0) == shim.INVALID and last(shim) == f"{prefix}x_dev is not memory of device 1{whose}"
    # the table form: a null optional argument and device-1 pointers pass
    assert table(shim, family, [good, None, other], [True, False, True]) == 0
    assert table(shim, family, [good, None, other], [True, True, True]) == shim.INVALID and last(shim) == f"{who}second_dev is null"
    assert table(shim, family, [good, unknown, other], [True, False, True]) == shim.INVALID
    assert last(shim) == f"{prefix}second_dev is not a device pointer"
    # the first bad entry in table order is the one reported
    assert table(shim, family, [dev0, None, host], [True, True, True]) == shim.INVALID
    assert last(shim) == f"{prefix}first_dev is not memory of device 1{whose}"
    assert table(shim, family, [good, host, None], [True, True, True]) == shim.INVALID
    assert last(shim) == f"{prefix}second_dev is not memory of device 1{whose}"
    assert events(shim) == []                             # a check synchronises and frees nothing


# ---- the blob frame ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefix", ["", "wg_norm_get_state: "])
def test_blob_get(shim, prefix):
    shim.fake_reset()
    total, n = shim.blob_header_bytes() + 40, C.c_size_t(0)
    assert shim.blob_get(prefix.encode(), 1, None, C.byref(n), total) == 0          # the size query: the size and nothing else
    assert n.value == total and events(shim) == [] and shim.fake_current() == 0
    buf, short = (C.c_char * total)(), C.c_size_t(total - 1)
    assert shim.blob_get(prefix.encode(), 1, buf, C.byref(short), total) == shim.INVALID
    assert last(shim) == prefix + "state buffer too small" and events(shim) == []
    assert shim.blob_get(prefix.encode(), 1, buf, C.byref(n), total) == 0
    assert events(shim) == [SYNC, COPY] and shim.fake_sync_device(0) == 1           # current and idle before the first copy


@pytest.mark.parametrize("prefix, not_ours", [("", "not a windgym state blob"), ("wg_curriculum_set_state: ", "not a curriculum state blob")])
def test_blob_set(shim, prefix, not_ours):
    import struct
    shim.fake_reset()
    hb = shim.blob_header_bytes()
    blob = struct.pack("<Iiii", shim.blob_magic(), 3, 2, 0) + bytes(40)
    call = lambda b, rows=3, cols=2: shim.blob_set(prefix.encode(), 1, b, len(b), not_ours.encode(), rows, cols)      # noqa: E731
    assert call(blob[:hb - 1]) == shim.INVALID and last(shim) == prefix + "state blob too small"
    wrong = struct.pack("<I", shim.blob_magic() ^ 1) + blob[4:]
    assert call(wrong) == shim.INVALID and last(shim) == prefix + not_ours
    assert call(blob, rows=4) == shim.INVALID and last(shim) == "shim: the blob is 3 x 2"          # the caller's own words
    assert events(shim) == [] and shim.fake_current() == 0                                            # a refused blob touches nothing
    assert call(blob) == 0
    assert events(shim) == [SYNC, COPY] and shim.fake_sync_device(0) == 1


def test_blob_frame_when_the_device_cannot_be_made_current(shim):
    shim.fake_reset()
    shim.fake_fail(SETDEVICE, 0, INVALID_DEVICE)
    total = shim.blob_header_bytes()
    buf, n = (C.c_char * total)(), C.c_size_t(total)
    assert shim.blob_get(b"", 1, buf, C.byref(n), total) == shim.HIP
    assert last(shim) == "hipSetDevice: invalid device ordinal" and events(shim) == []


def test_header_is_host_only():
    """No HIP include in the header or behind it: with the stand-ins in front of it, g++ reads it with no ROCm include path."""
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", CSRC, os.path.join(ROOT, "tests", "host_layer_shim.cpp")], check=True)
    for name in ("wg_host.h", "wg_devmem.h"):
        with open(os.path.join(CSRC, name)) as f:
            assert "#include <hip" not in f.read()


# ---- Python: binding.Handle and binding.tensor_ptr, no GPU and no library ----------------------------------------------------------
class StubLibrary:
    """Counts the calls of ``thing_destroy`` and ``thing_get_state``; the state is ``payload``."""

    def __init__(self, payload=b"", destroy_raises=False):
        self.payload, self.destroy_raises, self.destroyed, self.gets = payload, destroy_raises, [], []

    def thing_destroy(self, h):
        self.destroyed.append(h)
        if self.destroy_raises:
            raise RuntimeError("destroy failed")
        return 0

    def thing_get_state(self, h, buf, size_ref):
        size = size_ref._obj
        self.gets.append((h, None if buf is None else len(buf), size.value))
        if buf is not None:
            buf[:len(self.payload)] = self.payload
        size.value = len(self.payload)
        return 0


def make_handle(lib):
    from windgym_amd.binding import Handle

    class Thing(Handle):
        destroy = "thing_destroy"

        def __init__(self):
            self.L, self._h = lib, C.c_void_p(0x1234)

    return Thing()


def test_handle_close_is_idempotent():
    lib = StubLibrary()
    t = make_handle(lib)
    h = t._h
    t.close()
    assert t._h is None and lib.destroyed == [h]
    t.close()
    t.__del__()
    assert lib.destroyed == [h]


def test_handle_never_opened_has_nothing_to_close():
    from windgym_amd.binding import Handle
    t = Handle.__new__(Handle)          # a constructor that raised before it had a handle
    t.close()
    t.__del__()


def test_handle_del_swallows_a_failing_destroy():
    lib = StubLibrary(destroy_raises=True)
    t = make_handle(lib)
    t.__del__()
    assert len(lib.destroyed) == 1
    with pytest.raises(RuntimeError, match="destroy failed"):
        make_handle(lib).close()


def test_handle_blob_is_two_calls():
    lib = StubLibrary(payload=bytes(range(37)))
    t = make_handle(lib)
    assert t._blob("thing_get_state") == bytes(range(37))
    assert lib.gets == [(t._h, None, 0), (t._h, 37, 37)]          # the size with NULL, then a buffer of the size reported
    t.close()


def test_tensor_ptr_messages():
    import torch
    from windgym_amd.binding import device_tensor, tensor_ptr
    from windgym_amd.policy import device_tensor as reexported
    assert reexported is device_tensor
    cpu = torch.zeros(6, dtype=torch.float32)
    meta = torch.zeros((2, 3), dtype=torch.float32, device="meta")          # (stands for no tensor a library call could take either)
    cases = {"a non-tensor": [1.0] * 6, "a numpy array": cpu.numpy(), "a CPU tensor": cpu, "a meta tensor": meta,
             "a wrong dtype": cpu.double(), "a non-contiguous view": torch.zeros((6, 2))[:, 0], "a wrong numel": torch.zeros(5)}
    for what, x in cases.items():
        assert not device_tensor(x, torch.float32), what
        for kw in (dict(numel=6), dict(at_least=6), dict(shape=(6,)), dict(numel=6, device=torch.device("cpu"))):
            msg = f"rows(): out must be a contiguous float32 CUDA tensor of 6 elements ({what})"
            with pytest.raises(ValueError) as e:
                tensor_ptr(x, torch.float32, msg, **kw)
            assert str(e.value) == msg
