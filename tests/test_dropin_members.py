"""CPU: the drop-in's host record of its members (usearch_amd/csrc/members.hpp behind usearch_amd/csrc/dropin.hip) against the
model of tests/dropin_members_model.py, call for call through ctypes. Members are only staged on the host here
(USEARCH_AMD_IMMEDIATE_ADD=0) and every script stays within the entry points that do not reach the device in the states it visits:
no search, no filter, no sync, no save of a staged non-empty index, no isolate / compact after a removal (the GPU suites hold those).
After every call: the return value, the exact error string or its absence, `size`, `capacity`, and `contains` / `count` / `get` of
every key the script has used so far."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

from oracle import oraclebind
from tests import util
from tests.dropin_members_model import DUPLICATE, FREE, FREE_KEY, IN_USE, OUT_OF_ROOM, Members

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBRARY = os.path.join(ROOT, "usearch_amd", "lib", "libusearch_c.so")
COS, F32, I8 = 1, 1, 4  # usearch_metric_cos_k, usearch_scalar_f32_k, usearch_scalar_i8_k (c/usearch.h)
UNKNOWN_KIND = 99
EMPTY_IMAGE_BYTES = 112


class Options(C.Structure):  # usearch_init_options_t, c/usearch.h:64-110
    _fields_ = [("metric_kind", C.c_int), ("metric", C.c_void_p), ("quantization", C.c_int), ("dimensions", C.c_size_t),
                ("connectivity", C.c_size_t), ("expansion_add", C.c_size_t), ("expansion_search", C.c_size_t),
                ("multi", C.c_bool)]


@pytest.fixture(scope="module")
def lib():
    L = C.CDLL(LIBRARY)
    err = C.POINTER(C.c_char_p)
    L.usearch_init.restype = C.c_void_p
    L.usearch_init.argtypes = [C.POINTER(Options), err]
    for name in ("size", "capacity", "serialized_length", "isolate", "compact"):
        getattr(L, f"usearch_{name}").restype = C.c_size_t
        getattr(L, f"usearch_{name}").argtypes = [C.c_void_p, err]
    L.usearch_free.argtypes = [C.c_void_p, err]
    L.usearch_clear.argtypes = [C.c_void_p, err]
    L.usearch_reserve.argtypes = [C.c_void_p, C.c_size_t, err]
    L.usearch_add.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, err]
    L.usearch_contains.restype = C.c_bool
    L.usearch_contains.argtypes = [C.c_void_p, C.c_uint64, err]
    L.usearch_count.restype = C.c_size_t
    L.usearch_count.argtypes = [C.c_void_p, C.c_uint64, err]
    L.usearch_get.restype = C.c_size_t
    L.usearch_get.argtypes = [C.c_void_p, C.c_uint64, C.c_size_t, C.c_void_p, C.c_int, err]
    L.usearch_remove.restype = C.c_size_t
    L.usearch_remove.argtypes = [C.c_void_p, C.c_uint64, err]
    L.usearch_rename.restype = C.c_size_t
    L.usearch_rename.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, err]
    for name in ("save_buffer", "load_buffer", "view_buffer"):
        getattr(L, f"usearch_{name}").argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, err]
    L.usearch_metadata_buffer.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(Options), err]
    return L


@pytest.fixture(autouse=True)
def staged_on_the_host_only(monkeypatch):
    monkeypatch.setenv("USEARCH_AMD_IMMEDIATE_ADD", "0")  # read in `usearch_init`: an add never links on the device


REMOVED = (1003, 1010, 1011, 1027, 1040, 1058, 1059)


@pytest.fixture(scope="module")
def image(reference):
    """60 members of 4 f32 dimensions, seven of them removed, as the reference serializes them: slot i holds key 1000 + i."""
    bytes_, vectors, _ = util.build_image(60, 4, "cos", "f32", connectivity=4, remove=REMOVED)
    return np.ascontiguousarray(bytes_), np.ascontiguousarray(vectors, dtype=np.float32)


class Driver:
    """One index and its model, side by side."""

    def __init__(self, lib, dimensions=4, quantization="f32", multi=False, options=True):
        self.lib, self.dimensions, self.quantization = lib, dimensions, quantization
        self.err = C.c_char_p()
        self.used = set()
        self.model = Members(multi=multi)
        chosen = Options(COS, None, {"f32": F32, "i8": I8}[quantization], dimensions, 4, 16, 16, multi)
        self.index = lib.usearch_init(C.byref(chosen) if options else None, C.byref(self.err))
        assert self.index and not self.err.value
        self.keep = []  # buffers a view borrows

    def close(self):
        self.lib.usearch_free(self.index, C.byref(self.err))

    def error(self):
        """The error string of the call before, or None; cleared for the next call."""
        value, self.err = self.err.value, C.c_char_p()
        return value.decode() if value else None

    def stored(self, vector):
        """An f32 vector as the index keeps it."""
        if self.quantization == "f32":
            return vector.astype(np.float32).tobytes()
        return oraclebind.cast(vector.astype(np.float32), "f32", self.quantization, self.dimensions).tobytes()

    def exported(self, row):
        """A stored row as `usearch_get` hands it out in f32."""
        if self.quantization == "f32":
            return row
        return oraclebind.cast(np.frombuffer(row, dtype=np.uint8), self.quantization, "f32", self.dimensions).tobytes()

    def check(self):
        lib, model = self.lib, self.model
        assert lib.usearch_size(self.index, C.byref(self.err)) == model.size() and self.error() is None
        assert lib.usearch_capacity(self.index, C.byref(self.err)) == model.reported_capacity() and self.error() is None
        for key in sorted(self.used):
            count = model.count(key)
            assert lib.usearch_contains(self.index, key, C.byref(self.err)) == (count != 0) and self.error() is None, key
            assert lib.usearch_count(self.index, key, C.byref(self.err)) == count and self.error() is None, key
            for asked in {1, count + 1}:  # fewer than there are (for a multi-key) and more
                out = np.full((asked, self.dimensions), np.nan, dtype=np.float32)
                got = lib.usearch_get(self.index, key, asked, C.c_void_p(out.ctypes.data), F32, C.byref(self.err))
                assert self.error() is None
                expected = [self.exported(row) for row in model.get(key, asked)]
                assert got == len(expected), key
                assert [out[i].tobytes() for i in range(got)] == expected, key  # rows in slot order

    def reserve(self, capacity):
        self.lib.usearch_reserve(self.index, capacity, C.byref(self.err))
        assert self.error() is None
        self.model.reserve(capacity)
        self.check()

    def add(self, key, vector, kind=F32):
        vector = np.ascontiguousarray(vector, dtype=np.float32)
        self.lib.usearch_add(self.index, key, C.c_void_p(vector.ctypes.data), kind, C.byref(self.err))
        expected = "Unknown scalar kind!" if kind == UNKNOWN_KIND else self.model.add(key, self.stored(vector))
        assert self.error() == expected, key
        if key != FREE:
            self.used.add(key)
        self.check()
        return expected

    def remove(self, key):
        got = self.lib.usearch_remove(self.index, key, C.byref(self.err))
        assert self.error() is None and got == self.model.remove(key), key
        self.used.add(key)
        self.check()
        return got

    def rename(self, source, target):
        got = self.lib.usearch_rename(self.index, source, target, C.byref(self.err))
        expected, message = self.model.rename(source, target)
        assert self.error() == message and got == expected, (source, target)
        self.used.update(key for key in (source, target) if key != FREE)
        self.check()
        return got, message

    def clear(self):
        self.lib.usearch_clear(self.index, C.byref(self.err))
        assert self.error() is None
        self.model.clear()
        self.check()

    def open(self, how, image, vectors, removed=REMOVED):
        """`load_buffer` copies, `view_buffer` borrows: the members are the image's either way."""
        self.keep.append(image)
        getattr(self.lib, f"usearch_{how}")(self.index, C.c_void_p(image.ctypes.data), len(image), C.byref(self.err))
        assert self.error() is None
        keys = [FREE if 1000 + slot in removed else 1000 + slot for slot in range(len(vectors))]
        self.model.open_image(keys, [row.tobytes() for row in vectors], multi=False)
        self.used.update(1000 + slot for slot in range(len(vectors)))
        self.check()

    def serialized(self):
        """Only where no device is needed: the index is still its image, or has no slot at all."""
        assert not self.model.staged or not self.model.slots
        length = self.lib.usearch_serialized_length(self.index, C.byref(self.err))
        assert self.error() is None
        out = np.zeros(length, dtype=np.uint8)
        self.lib.usearch_save_buffer(self.index, C.c_void_p(out.ctypes.data), length, C.byref(self.err))
        assert self.error() is None
        self.lib.usearch_save_buffer(self.index, C.c_void_p(out.ctypes.data), length - 1, C.byref(self.err))
        assert self.error() == "Buffer is too small"
        return out.tobytes()

    def nothing_to_drop(self):
        """`isolate` / `compact` with nobody removed: nothing to do, and nothing about the members changes."""
        assert self.model.size() == len(self.model.slots)
        for name in ("isolate", "compact"):
            assert getattr(self.lib, f"usearch_{name}")(self.index, C.byref(self.err)) == 0 and self.error() is None
        self.check()


def empty_image(dimensions, quantization, multi, connectivity=4):
    """What an index without nodes serializes to (index_dense.hpp:995-1062 with zero rows): the matrix dimensions, the 64-byte head,
    the five-word graph header."""
    scalar, width = {"f32": (11, 4), "i8": (23, 1)}[quantization]  # the on-disk scalar kinds, index_plugins.hpp:113-159
    head = b"usearch" + struct.pack("<3H", 2, 21, 0) + bytes([ord("c"), scalar, 14, 15]) + bytes(16) + struct.pack("<Q", dimensions)
    head += bytes([1 if multi else 0])
    return struct.pack("<II", 0, dimensions * width) + head.ljust(64, b"\0") + struct.pack("<5Q", 0, connectivity, 2 * connectivity, 0, 0)


def random_script(driver, rng, keys, steps):
    """`steps` calls drawn from add / remove / rename over a small pool of keys, so that every kind of collision comes up. A multi-key
    removal frees several slots in an order no rule fixes: the adds that retake them carry one and the same member (see the model)."""
    model, fill = driver.model, None
    for _ in range(steps):
        if model.filling is not None:
            driver.add(model.filling[0], fill)
            continue
        draw, key = rng.random(), int(rng.choice(keys))
        if draw < 0.45:
            fill = rng.standard_normal(driver.dimensions).astype(np.float32)
            driver.add(key, fill)
        elif draw < 0.75:
            driver.remove(key)
        else:
            driver.rename(key, int(rng.choice(keys)))


@pytest.mark.parametrize("quantization", ["f32", "i8"])
def test_members_from_init(lib, quantization):
    """(a) One key per member: capacity, the refusals by name, freed slots as room, renames."""
    rng = np.random.default_rng(11)
    driver = Driver(lib, quantization=quantization)
    vector = lambda: rng.standard_normal(4).astype(np.float32)
    assert driver.add(1, vector()) == OUT_OF_ROOM  # nothing reserved yet
    driver.reserve(12)
    for key in range(1, 13):
        assert driver.add(key, vector()) is None
    assert driver.add(13, vector()) == OUT_OF_ROOM  # full, and full comes before duplicate
    assert driver.add(5, vector()) == OUT_OF_ROOM
    driver.reserve(14)
    assert driver.add(5, vector()) == DUPLICATE
    assert driver.add(FREE, vector()) == FREE_KEY
    assert driver.add(20, vector(), kind=UNKNOWN_KIND) == "Unknown scalar kind!"
    out = np.zeros(4, dtype=np.float32)
    assert lib.usearch_get(driver.index, 5, 1, C.c_void_p(out.ctypes.data), UNKNOWN_KIND, C.byref(driver.err)) == 0
    assert driver.error() == "Unknown scalar kind!"
    assert driver.add(13, vector()) is None and driver.add(14, vector()) is None
    assert driver.add(15, vector()) == OUT_OF_ROOM
    # freed slots are room, and only as long as they last
    assert driver.remove(3) == 1 and driver.remove(9) == 1 and driver.remove(3) == 0
    assert driver.add(15, vector()) is None and driver.add(3, vector()) is None
    assert driver.add(16, vector()) == OUT_OF_ROOM
    assert driver.rename(1, 2) == (0, IN_USE)
    assert driver.rename(1, 1) == (0, IN_USE)
    assert driver.rename(9, 30) == (0, None)  # absent
    assert driver.rename(1, FREE) == (0, FREE_KEY)
    assert driver.rename(1, 9) == (1, None)
    random_script(driver, rng, np.arange(1, 25), 300)
    # an image that is refused takes nothing away from members that are staged
    lib.usearch_load_buffer(driver.index, C.c_void_p(vector().ctypes.data), 7, C.byref(driver.err))
    assert driver.error() == "Failed to read 32-bit dimensions of the matrix"
    driver.check()
    driver.clear()
    assert driver.add(1, vector()) is None  # the capacity stays
    driver.close()


def test_members_of_a_multi_index(lib):
    """(a) Several rows per key: `get` in slot order, which also shows WHICH freed slot an add takes: the oldest."""
    rng = np.random.default_rng(12)
    driver = Driver(lib, multi=True)
    vector = lambda: rng.standard_normal(4).astype(np.float32)
    driver.reserve(10)
    for key in (1, 2, 3, 1, 2, 3, 1, 2, 3):  # slots 0..8: three rows per key, interleaved
        assert driver.add(key, vector()) is None
    assert driver.add(4, vector()) is None and driver.add(5, vector()) == OUT_OF_ROOM
    assert driver.rename(4, 6) == (1, None)
    assert driver.remove(6) == 1  # frees slot 9 …
    assert driver.rename(3, 7) == (3, None)
    first, second = vector(), vector()
    assert driver.add(8, first) is None  # … which the next add takes; the one after finds no room
    assert driver.add(8, second) == OUT_OF_ROOM
    assert driver.remove(8) == 1 and driver.remove(1) == 3  # the ring: slot 9, then slots 0, 3, 6 in some order
    assert driver.add(9, first) is None  # slot 9, the oldest
    same = vector()
    for _ in range(3):
        assert driver.add(9, same) is None  # slots 0, 3, 6: `get` now starts with them, and ends with slot 9
    assert driver.model.get(9, 4) == [same.tobytes()] * 3 + [first.tobytes()]
    assert driver.add(9, same) == OUT_OF_ROOM
    assert driver.rename(2, 9) == (3, None)  # a multi-index merges on rename
    random_script(driver, rng, np.arange(1, 9), 300)
    driver.close()


@pytest.mark.parametrize("how", ["load_buffer", "view_buffer"])
def test_members_of_an_image(lib, image, how):
    """(b) An index that is still its image: read before anything stages it, saved byte for byte, its tombstones as room."""
    image_bytes, vectors = image
    rng = np.random.default_rng(13)
    vector = lambda: rng.standard_normal(4).astype(np.float32)
    options, err = Options(), C.c_char_p()
    lib.usearch_metadata_buffer(C.c_void_p(image_bytes.ctypes.data), len(image_bytes), C.byref(options), C.byref(err))
    assert not err.value
    assert (options.metric_kind, options.quantization, options.dimensions, options.connectivity, options.multi) == (COS, F32, 4, 4, False)
    lib.usearch_metadata_buffer(C.c_void_p(image_bytes.ctypes.data), 7, C.byref(options), C.byref(err))
    assert err.value == b"Failed to read 32-bit dimensions of the matrix"

    driver = Driver(lib, options=False)  # an empty shell to load into
    driver.open(how, image_bytes, vectors)  # `check` reads every key: `get`, `count`, `contains` from the image
    assert driver.model.size() == 53 and driver.model.reported_capacity() == 60
    assert driver.serialized() == image_bytes.tobytes()
    assert driver.rename(1003, 2000) == (0, None)  # removed in the image
    assert driver.rename(1000, 1001) == (0, IN_USE)
    assert not driver.model.staged and driver.serialized() == image_bytes.tobytes()
    assert driver.rename(1000, 2000) == (1, None)  # the first change: keys and rows leave the image
    # at capacity, the seven tombstones are room for exactly seven
    assert driver.add(1001, vector()) == DUPLICATE
    for key in range(3000, 3007):
        assert driver.add(key, vector()) is None
    assert driver.add(3007, vector()) == OUT_OF_ROOM
    random_script(driver, rng, np.arange(1000, 1070), 300)

    # the same from an untouched image: the very first call is an add at capacity
    driver.open(how, image_bytes, vectors)
    for key in range(3000, 3007):
        assert driver.add(key, vector()) is None
    assert driver.add(3007, vector()) == OUT_OF_ROOM
    # … and with room to spare, the tombstones still go first: 7 + 2 more
    driver.open(how, image_bytes, vectors)
    driver.reserve(62)
    for key in range(3000, 3009):
        assert driver.add(key, vector()) is None
    assert driver.add(3009, vector()) == OUT_OF_ROOM

    driver.clear()
    assert driver.serialized() == empty_image(4, "f32", False)
    assert driver.add(1, vector()) is None and driver.add(1, vector()) == DUPLICATE
    random_script(driver, rng, np.arange(1, 30), 200)
    driver.close()


def test_an_image_nobody_was_removed_from_has_nothing_to_drop(lib, reference):
    image_bytes, vectors, _ = util.build_image(20, 4, "cos", "f32", connectivity=4)
    image_bytes = np.ascontiguousarray(image_bytes)
    driver = Driver(lib, options=False)
    driver.open("load_buffer", image_bytes, np.ascontiguousarray(vectors, dtype=np.float32), removed=())
    driver.nothing_to_drop()
    assert driver.serialized() == image_bytes.tobytes()
    damaged = image_bytes[:-5].copy()
    driver.lib.usearch_load_buffer(driver.index, C.c_void_p(damaged.ctypes.data), len(damaged), C.byref(driver.err))
    assert driver.error() == "Failed to pull nodes from the stream"
    # a refused image leaves an empty index of the same configuration behind
    assert lib.usearch_size(driver.index, C.byref(driver.err)) == 0 and lib.usearch_capacity(driver.index, C.byref(driver.err)) == 20
    assert driver.serialized() == empty_image(4, "f32", False)
    driver.clear()
    driver.close()


@pytest.mark.parametrize("quantization,multi", [("f32", False), ("i8", True)])
def test_the_empty_index(lib, quantization, multi):
    """(c) 112 bytes of headers, from an index that never staged anything and from a staged one that `clear` emptied."""
    rng = np.random.default_rng(14)
    driver = Driver(lib, dimensions=6, quantization=quantization, multi=multi)
    expected = empty_image(6, quantization, multi)
    assert len(expected) == EMPTY_IMAGE_BYTES
    assert lib.usearch_serialized_length(driver.index, C.byref(driver.err)) == EMPTY_IMAGE_BYTES and driver.error() is None
    assert driver.serialized() == expected
    driver.nothing_to_drop()
    driver.reserve(4)
    assert driver.serialized() == expected
    for key in (1, 2, 3):
        assert driver.add(key, rng.standard_normal(6).astype(np.float32)) is None
    driver.remove(2)
    driver.clear()
    assert driver.serialized() == expected
    driver.nothing_to_drop()
    driver.close()
