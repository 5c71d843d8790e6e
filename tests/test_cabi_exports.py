"""CPU-only: the ctypes binding is derived from include/g2v.h, the derived struct layouts are the C compiler's, and the library
exports exactly the functions the header declares (no compute calls)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from gesture2vec_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "g2v.h")

c_fp, c_i64, c_int, c_f, c_sz, c_u64 = C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_size_t, C.c_uint64

# The only hand-typed signatures left: they check the PARSER (every mapping rule at least once), not the header.
PINNED_SIGS = {
    "g2v_linear_fwd": (c_int, [c_fp, c_i64, c_int, c_i64, c_i64, c_fp, c_f, c_fp, c_fp, c_fp, c_i64,
                               c_int, c_int, c_int, c_int, c_fp]),
    "g2v_clip_adam_step_readback": (c_int, [c_fp, c_fp, c_fp, c_fp, c_i64, c_fp, c_fp, c_fp, c_f, c_f, c_f, c_f, c_f, c_f,
                                            c_fp, c_fp, c_fp, c_fp, c_fp]),
    "g2v_kmeans_pp_step": (c_int, [c_fp, c_i64, c_int, c_fp, C.POINTER(c_i64), C.POINTER(C.c_double), c_int, c_fp, c_fp, c_fp, c_sz,
                                   c_fp]),
    "g2v_kmeans_tolerance": (c_int, [c_fp, c_i64, c_int, C.c_double, c_fp, c_fp, c_sz, c_fp]),
    "g2v_linear_bwd_weight_deferred": (c_int, [C.POINTER(_lib.WgradItem), c_int, c_i64, c_i64, c_int, c_i64, c_i64, c_fp, c_int, c_int,
                                               c_int, c_int, c_fp, c_sz, C.POINTER(_lib.WgradPending), c_fp]),
    "g2v_dec_rollout_fwd": (c_int, [c_fp, c_fp, C.POINTER(_lib.DecWeights), C.POINTER(_lib.DecSaved), c_fp, c_fp, c_f,
                                    c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_fp, c_sz, c_fp]),
    "g2v_gru_seq_route": (c_int, [c_int] * 10),
    "g2v_vq_assign_route": (c_int, [c_int] * 7),
    "g2v_linear_route": (c_int, [c_int] * 9 + [c_i64] * 4 + [c_int] * 2),
    "g2v_attn_code_rollout_route": (c_int, [c_int] * 12),
    "g2v_ctx_destroy": (None, [C.c_void_p]),
    "g2v_version": (C.c_char_p, []),
    "g2v_keep_mask": (c_int, [c_fp, c_i64, c_f, c_u64, c_fp, c_fp]),
    "g2v_silhouette_samples": (c_int, [c_fp, c_i64, c_fp, c_i64, c_int, c_int, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_sz, c_fp]),
}
PINNED_FIELDS = {
    "GruDirBwd": ([(n, c_fp) for n in ("d_hs", "d_hn", "hs", "h0", "gates", "w_hh", "dgi", "dgh", "dh0")] + [("reverse", c_int)] +
                  [(n, c_fp) for n in ("w_ih", "dx")] + [("in_dim", c_int)] +
                  [(n, c_fp) for n in ("x", "dw_hh", "db_hh", "dw_ih", "db_ih", "wslab")] +
                  [(n, c_fp) for n in ("hn_z", "hn_q", "hn_gloss")] + [("hn_coef", c_f)] +
                  [("dgi_row_off", C.POINTER(C.c_int32))]),
    "WgradPending": ([("slab_w", c_fp * 4), ("out_w", c_fp * 4), ("slab_b", c_fp * 4), ("out_b", c_fp * 4), ("n", c_i64),
                      ("nb", c_i64)] + [(n, c_int) for n in ("nsplit", "nprob", "accumulate", "reserved")]),
}
STRUCT_NAMES = ("DecWeights", "DecSaved", "GruDir", "GruDirBwd", "WgradItem", "WgradPending", "DecGrads", "CodeDecWeights",
                "CodeDecSaved", "CodeDecGrads")


def declared_symbols():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(g2v_[a-z0-9_]+)\s*\(", src)))


def test_header_and_binding_agree():
    decl = declared_symbols()
    assert decl, "no declarations parsed"
    assert sorted(_lib.EXPORTS) == decl
    assert len(decl) == len(_lib.EXPORTS)            # (no function declared twice)


@pytest.mark.parametrize("name", sorted(PINNED_SIGS))
def test_pinned_signature(name):
    res, args = _lib._SIGS[name]
    want_res, want_args = PINNED_SIGS[name]
    assert res is want_res
    assert len(args) == len(want_args) and all(a is w for a, w in zip(args, want_args)), (args, want_args)


@pytest.mark.parametrize("name", sorted(PINNED_FIELDS))
def test_pinned_struct_fields(name):
    got, want = getattr(_lib, name)._fields_, PINNED_FIELDS[name]
    assert [n for n, _ in got] == [n for n, _ in want]
    assert all(g is w for (_, g), (_, w) in zip(got, want)), (got, want)


def test_structs_and_constants_keep_their_names():
    assert sorted(cls.__name__ for cls in _lib.STRUCTS.values()) == sorted(STRUCT_NAMES)
    for cname, cls in _lib.STRUCTS.items():
        assert getattr(_lib, cls.__name__) is cls and cls.__doc__ == cname and issubclass(cls, C.Structure)
    assert (_lib.OPT_PERSISTENT, _lib.OPT_GRU_CLUSTER, _lib.OPT_SMALLM_ROWS, _lib.OPT_GRU_RESIDENT_ROWS,
            _lib.OPT_GRU_RESIDENT_BWD, _lib.OPT_PRECLEAR_NOTES) == (1, 2, 3, 4, 5, 6)
    assert (_lib.OK, _lib.ERR_ARG, _lib.ERR_LAUNCH, _lib.ERR_WORKSPACE, _lib.ERR_UNSUPPORTED) == (0, -1, -2, -3, -4)
    assert (_lib.WGRAD_ACCUMULATE, _lib.WGRAD_BF16X3, _lib.WGRAD_PENDING_MAX, _lib.VQ_BX_EXACT) == (1, 2, 8, 1)
    assert "HOST" not in _lib.CONSTANTS and "G2V_HOST" not in _lib.CONSTANTS      # a marker, not a value


def _host_cc():
    for cand in ("cc", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang"),
                 os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "clang")):
        path = shutil.which(cand)
        if path:
            return path
    pytest.fail("no host C compiler (cc, or the clang that ships with ROCm): the struct layouts cannot be checked")


def test_struct_layout_is_the_compilers(tmp_path):
    """sizeof and every offsetof, as a C compiler sees include/g2v.h, against the ctypes classes derived from it"""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "g2v.h"', "int main(void) {"]
    want = []
    for cname, cls in _lib.STRUCTS.items():
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        want.append(f"{cname} {C.sizeof(cls)}")
        for fname, _ in cls._fields_:
            lines.append(f'  printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
            want.append(f"{cname}.{fname} {getattr(cls, fname).offset}")
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([_host_cc(), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")[:-1]
    assert len(_lib.STRUCTS) == 10 and got == want
    assert sorted(C.sizeof(cls) for cls in _lib.STRUCTS.values()) == [32, 112, 112, 128, 136, 152, 160, 160, 160, 192]


def test_library_exports_every_declared_symbol():
    lib = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in declared_symbols():
        assert hasattr(raw, name), f"{name} not exported by libg2v_hip.so"
    assert b"g2v" in lib.g2v_version()


def test_header_declares_every_exported_symbol():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    exported = {s for s in exported if re.match(r"^g2v_", s) and not re.match(r"^g2v_internal_", s)}
    assert exported, "nm listed no g2v_ symbol"
    assert sorted(exported - set(_lib.EXPORTS)) == []


@pytest.mark.parametrize("text, named", [
    ("int g2v_frobnicate(const float* x, foo_t n, g2v_stream_t stream);", "g2v_frobnicate"),          # unknown type
    ("#define G2V_N 4\ntypedef struct { float* rows[G2V_N]; int n; } g2v_bad_bound;", "rows[G2V_N]"),   # non-literal array bound
    ("int g2v_f(int n)\nint g2v_g(int n);", "g2v_f"),                                                  # (a lost semicolon)
    ("#define G2V_SCALE 1.5f", "G2V_SCALE"),                                                           # (not an integer)
])
def test_malformed_declarations_raise_and_are_named(text, named):
    prelude = "typedef void* g2v_stream_t;\n"
    assert _lib.parse_header(prelude + "int g2v_fine(const float* x, g2v_stream_t stream);")[0]["g2v_fine"] == (c_int, [c_fp, c_fp])
    with pytest.raises(_lib.G2VLibraryError) as e:
        _lib.parse_header(prelude + text)
    assert named in str(e.value)


def test_argument_errors_are_reported_not_thrown():
    lib = _lib.load()
    rc = lib.g2v_vq_code_sqnorm(None, None, 4, 4, None)
    assert rc == -1
    assert b"null" in lib.g2v_last_error()
    assert lib.g2v_vq_assign_blocks(4096) == 256
    assert lib.g2v_linear_bwd_weight_workspace(1000, 64, 192) > 0
