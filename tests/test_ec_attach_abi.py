"""CPU tests (-m "not gpu") of the ABI that bfcg_ec_attach and the resident count table add: the symbols, their declarations, the refusal
that needs no GPU, and the host table functions with the drop hook in place (nothing is registered without a GPU: one relaxed load)."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {
    "bfcg_ec_attach": ("bfcg_ec_t *", "(bfcg_ctx_t *ctx, const bfc_opt_t *opt, uint64_t max_pos, uint64_t max_reads)"),
    "bfcg_ec_retry_reads": ("uint64_t", "(bfcg_ec_t *e)"),
    "bfcg_ec_adopted": ("int", "(bfcg_ec_t *e)"),
    "bfcg_export_table_resident": ("bfc_ch_t *", "(bfcg_ctx_t *c)"),
}


def test_new_symbols_resolve_with_the_declared_signatures(gpu_lib):
    from bfc_amd import _lib
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "bfc_gpu.h")).read()
    for name, (ret, args) in NEW.items():
        assert hasattr(L, name)
        assert re.search(r"^%s\s*%s%s;" % (re.escape(ret), name, re.escape(args)), hdr, re.M), name
    S = _lib.SYMBOLS
    assert S["bfcg_ec_attach"] == (C.c_void_p, [C.c_void_p, C.POINTER(_lib.BfcOpt), C.c_uint64, C.c_uint64])
    assert S["bfcg_ec_retry_reads"] == (C.c_uint64, [C.c_void_p])
    assert S["bfcg_ec_adopted"] == (C.c_int, [C.c_void_p])
    assert S["bfcg_export_table_resident"] == (C.c_void_p, [C.c_void_p])


def test_attach_to_nothing_is_refused(gpu_lib):
    L = gpu_lib._lib.load()
    o = gpu_lib.bfc_opt_init(); o.k = 31
    assert L.bfcg_ec_attach(None, C.byref(o), 1 << 20, 1 << 10) is None
    assert b"bfcg_ec_attach" in L.bfcg_last_error()


def test_host_table_works_with_the_drop_hook(gpu_lib):
    """bfc_ch_init / bfc_ch_insert / bfc_ch_destroy call the (weak) bfcg_resident_drop: with an empty registry they behave as before"""
    L = gpu_lib._lib.load()
    t = gpu_lib.HostTable.init(31, 20)
    rng = np.random.default_rng(9)
    keys = rng.integers(0, 1 << 31, (500, 2), dtype=np.uint64)
    for y0, y1 in keys:
        assert t.insert(int(y0), int(y1), 1) == 0
    assert t.count() == len(np.unique(keys, axis=0))
    y0, y1 = (int(v) for v in keys[0])
    assert t.get(y0, y1) & 0xff >= 1
    L.bfcg_resident_drop(t.ptr)                                  # nothing registered: a no-op
    assert t.get(y0, y1) & 0xff >= 1
    t.close()
    t2 = gpu_lib.HostTable.init(31, 20)                          # an address may come back: nothing stale behind it
    assert t2.count() == 0 and t2.get(y0, y1) == -1
    t2.close()
