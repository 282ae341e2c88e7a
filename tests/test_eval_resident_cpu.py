"""CPU checks of the resident eval pass's C ABI and engine surface (no GPU): libtgnx exports
tgnx_tgn_eval_step_resident, tgnx/_lib.py binds it with the header's argument list, the eval cursor has its own
control word, and TgnEngine carries the calls named after their train counterparts."""
import ctypes
import os
import re

from conftest import ROOT


def test_library_exports_eval_step_resident():
    from tgnx import _lib
    L = _lib.lib()
    assert hasattr(L, "tgnx_tgn_eval_step_resident")
    res, args = _lib.SIGNATURES["tgnx_tgn_eval_step_resident"]
    P, i64, i32, u64, vp = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_uint64, ctypes.c_void_p
    assert res is ctypes.c_int
    # (cfg, buf, split_lo, split_hi, batch, Kn, rank, world, base_seed, rr_ev, stream)
    assert args == [P, P, i64, i64, i64, i32, i32, i32, u64, P, vp]
    assert L.tgnx_tgn_eval_step_resident.argtypes == args


def test_header_declares_entry_point_and_cursor_word():
    hdr = open(os.path.join(ROOT, "include", "tgnx.h")).read()
    m = re.search(r"int tgnx_tgn_eval_step_resident\(([^;]*)\);", hdr)
    assert m, "include/tgnx.h does not declare tgnx_tgn_eval_step_resident"
    names = [a.split()[-1].lstrip("*") for a in m.group(1).replace("\n", " ").split(",")]
    assert names == ["cfg", "buf", "split_lo", "split_hi", "batch", "Kn", "rank", "world", "base_seed", "rr_ev", "stream"]
    w = re.search(r"#define TGNX_CTL_EVAL_NB (\d+)", hdr)
    words = int(re.search(r"#define TGNX_CTL_WORDS (\d+)", hdr).group(1))
    used = {int(x) for x in re.findall(r"#define TGNX_CTL_(?!WORDS|EVAL_NB)[A-Z_]+ (\d+)", hdr)} | {15}
    assert w and int(w.group(1)) < words and int(w.group(1)) not in used
    assert "tests/test_gpu_tgn_eval_resident.py" in hdr


def test_null_arguments_are_rejected_without_a_device():
    from tgnx import _lib
    L = _lib.lib()
    rc = L.tgnx_tgn_eval_step_resident(None, None, 0, 0, 1, 1, 0, 1, 0, None, None)
    assert rc != 0 and L.tgnx_last_error()


def test_engine_has_the_resident_eval_calls():
    from tgnx.tgn import TgnEngine
    for name in ("bind_eval_resident", "eval_resident_step", "capture_eval", "replay_eval_n", "begin_eval", "eval_rr",
                 "eval_mrr"):
        assert callable(getattr(TgnEngine, name, None)), name
