"""CPU suite: the ctypes binding is derived from include/dagr_hip.h (dagr_amd/_header.py).  The reader on every shape of
declaration the header contains, the derived structure layouts against the C compiler's own sizeof / offsetof, and the
whole header against the built library."""
import ctypes
import os
import shutil
import subprocess
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_void_p

import numpy as np
import pytest

from dagr_amd import _lib
from dagr_amd._header import Header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fields(cls):
    return [(n, t) for n, t in cls._fields_]


# ------------------------------------------------------------------------------------------------ 1. the reader
def test_reader_functions():
    h = Header("""
        #ifndef X_H
        #define X_H
        #include <stdint.h>
        #ifdef __cplusplus
        extern "C" {
        #endif
        typedef struct { int32_t width; int64_t max_events; } dagr_graph_desc;
        const char *dagr_last_error(void);
        /* a comment between declarations; with a semicolon */
        int dagr_version(void);
        const int32_t *dagr_count_ptr(const dagr_graph_desc *desc, void *workspace);
        void dagr_bounds(int32_t *max_gt, int32_t *max_dt);
        int dagr_format(const int16_t *xy /*[N,2]*/, const int8_t *p /*[N], a comma*/, int64_t N,
                        float *pos_out /*[N,3]*/, const void *batch, void *stream);  // trailing
        size_t dagr_bytes(int32_t n_thr, int64_t n_cols);
        int dagr_acc(const uint8_t *dtm, const double *rec_thrs, double eps, size_t workspace_bytes, float atol);
        int32_t dagr_passes(int32_t cin, int32_t);
        #define DAGR_MAX 256
        #ifdef __cplusplus
        }
        #endif
        #endif
    """)
    G = h.structs["dagr_graph_desc"]
    assert h.functions == {
        "dagr_last_error": (c_char_p, []),
        "dagr_version": (c_int, []),
        "dagr_count_ptr": (c_void_p, [POINTER(G), c_void_p]),
        "dagr_bounds": (None, [c_void_p, c_void_p]),
        "dagr_format": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
        "dagr_bytes": (c_size_t, [c_int32, c_int64]),
        "dagr_acc": (c_int, [c_void_p, c_void_p, c_double, c_size_t, c_float]),
        "dagr_passes": (c_int32, [c_int32, c_int32]),
    }
    assert list(h.functions) == ["dagr_last_error", "dagr_version", "dagr_count_ptr", "dagr_bounds", "dagr_format",
                                 "dagr_bytes", "dagr_acc", "dagr_passes"]


def test_reader_structs_and_enums():
    h = Header("""
        typedef enum { DAGR_OK = 0, DAGR_ERR_INVALID_ARG = -1, DAGR_ERR_HIP = -2 } dagr_status;
        enum { DAGR_FLOPS_ZERO = 0, DAGR_FLOPS_CONV = 1, DAGR_FLOPS_NEXT, DAGR_FLOPS_HEX = 0x10 };
        typedef struct {
            int32_t width;          /* W, pixels */
            int32_t gx, gy;         /* two declarators */
            float vx, vy;
            int64_t max_events;
        } dagr_graph_desc;
        typedef struct dagr_head_scale {
            const int32_t *n_ptr; int32_t n_max;
            const int32_t *rowptr, *col, ld, *code;
            const float *cnn[3]; int32_t cnn_stride[3][4];
            int32_t crop_lo[2], crop_hi[2];
            const dagr_graph_desc *gdesc; void *graph_ws; double eps;
        } dagr_head_scale;
        dagr_status dagr_use(const dagr_head_scale *scale0, const dagr_graph_desc *desc);
    """)
    assert h.enums == {"DAGR_OK": 0, "DAGR_ERR_INVALID_ARG": -1, "DAGR_ERR_HIP": -2, "DAGR_FLOPS_ZERO": 0,
                       "DAGR_FLOPS_CONV": 1, "DAGR_FLOPS_NEXT": 2, "DAGR_FLOPS_HEX": 16}
    assert list(h.structs) == ["dagr_graph_desc", "dagr_head_scale"]
    G, S = h.structs["dagr_graph_desc"], h.structs["dagr_head_scale"]
    assert issubclass(G, ctypes.Structure) and (G.__name__, S.__name__) == ("GraphDesc", "HeadScale")
    assert _fields(G) == [("width", c_int32), ("gx", c_int32), ("gy", c_int32), ("vx", c_float), ("vy", c_float),
                          ("max_events", c_int64)]
    assert _fields(S) == [("n_ptr", c_void_p), ("n_max", c_int32), ("rowptr", c_void_p), ("col", c_void_p),
                          ("ld", c_int32), ("code", c_void_p), ("cnn", c_void_p * 3), ("cnn_stride", (c_int32 * 4) * 3),
                          ("crop_lo", c_int32 * 2), ("crop_hi", c_int32 * 2), ("gdesc", POINTER(G)),
                          ("graph_ws", c_void_p), ("eps", c_double)]
    s = S()
    s.cnn_stride[2][3] = 7                                           # row-major: three rows of four
    assert ctypes.sizeof(s.cnn_stride) == 48 and len(s.cnn_stride) == 3 and len(s.cnn_stride[0]) == 4
    assert np.frombuffer(bytes(s.cnn_stride), np.int32)[2 * 4 + 3] == 7
    assert h.functions == {"dagr_use": (c_int, [POINTER(S), POINTER(G)])}


@pytest.mark.parametrize("snippet, named", [
    ("int dagr_ok(int32_t n);\nint dagr_bad(uint16_t n, void *stream);", "dagr_bad(uint16_t n, void *stream)"),
    ("int dagr_bad(unsigned int n);", "dagr_bad(unsigned int n)"),
    ("long long dagr_bad(void);", "long long dagr_bad(void)"),
    ("int dagr_bad(float **rows);", "dagr_bad(float **rows)"),
    ("int dagr_bad(float rows[4]);", "dagr_bad(float rows[4])"),
    ("int dagr_bad(void x);", "dagr_bad(void x)"),
    ("wchar_t *dagr_bad(void);", "wchar_t *dagr_bad(void)"),
    ("int dagr_bad(const dagr_nowhere *desc);", "dagr_bad(const dagr_nowhere *desc)"),
    ("typedef struct { int32_t a; half b; } dagr_bad;", "half b"),
    ("typedef struct { int32_t a; float (*fn)(int); } dagr_bad;", "dagr_bad"),
    ("typedef struct { int32_t a : 3; } dagr_bad;", "int32_t a : 3"),
    ("typedef struct { struct { int32_t a; } in; } dagr_bad;", "struct { int32_t a; } in"),
    ("struct dagr_bad { int32_t a; };", "struct dagr_bad"),
    ("typedef struct dagr_tag { int32_t a; } dagr_bad;", "dagr_tag"),
    ("enum { DAGR_A = 1 << 2 };", "DAGR_A = 1 << 2"),
    ("typedef int32_t dagr_bad;", "typedef int32_t dagr_bad"),
    ("int dagr_twice(void);\nint dagr_twice(void);", "dagr_twice"),
])
def test_reader_raises_and_names_what_it_cannot_read(snippet, named):
    with pytest.raises(ValueError) as e:
        Header(snippet)
    assert named in str(e.value), str(e.value)


# ------------------------------------------------------------------------------------------------ 2. the compiler's layout
def _host_compiler():
    """clang of ROCm's LLVM: the compiler hipcc drives for host code."""
    roots = [os.environ.get("ROCM_PATH"), "/opt/rocm"]
    hipcc = shutil.which("hipcc")
    if hipcc:
        roots.insert(1, os.path.dirname(os.path.dirname(os.path.realpath(hipcc))))
    for root in filter(None, roots):
        for rel in ("lib/llvm/bin/clang", "llvm/bin/clang"):
            if os.access(os.path.join(root, rel), os.X_OK):
                return os.path.join(root, rel)
    return shutil.which("amdclang") or shutil.which("clang")


@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    """{"dagr_x": sizeof, "dagr_x.field": offsetof, ...} of every struct of the header, as the host compiler lays them
    out: a host-only program generated from the parsed field lists, compiled and run once."""
    cc = _host_compiler()
    assert cc, "no host C compiler found (ROCm's LLVM clang)"
    lines = ['#include <stdio.h>', '#include "dagr_hip.h"', "int main(void) {"]
    for name, cls in _lib.STRUCTS.items():
        lines.append(f'    printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'    printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f, _ in cls._fields_]
    lines += ["    return 0;", "}", ""]
    d = tmp_path_factory.mktemp("layout")
    (d / "layout.c").write_text("\n".join(lines))
    subprocess.run([cc, "-x", "c", "-std=c11", "-I", os.path.join(ROOT, "include"),
                    str(d / "layout.c"), "-o", str(d / "layout")], check=True, capture_output=True, text=True)
    out = subprocess.run([str(d / "layout")], check=True, capture_output=True, text=True).stdout
    return {k: int(v) for k, v in (ln.split() for ln in out.splitlines())}


def test_struct_layout_matches_the_compiler(c_layout):
    derived = {}
    for name, cls in _lib.STRUCTS.items():
        derived[name] = ctypes.sizeof(cls)
        derived.update({f"{name}.{f}": getattr(cls, f).offset for f, _ in cls._fields_})
    assert len(_lib.STRUCTS) == 8 and len(derived) > 130
    assert derived == c_layout


# ------------------------------------------------------------------------------------------------ 3. the whole header
def test_whole_header_is_bound(c_layout):
    src = open(os.path.join(ROOT, "include", "dagr_hip.h")).read()
    h = Header(src)
    assert set(h.functions) == set(_lib.SIGNATURES) and len(h.functions) >= 89
    L = _lib.lib()
    for name, (restype, argtypes) in _lib.SIGNATURES.items():
        fn = getattr(L, name)                                        # AttributeError: declared but not exported
        assert (fn.restype, list(fn.argtypes)) == (restype, argtypes), name
    # every struct has its class, under the name the package has always used
    assert sorted(h.structs) == sorted(_lib.STRUCTS)
    want = {"dagr_pool_desc": "PoolDesc", "dagr_graph_desc": "GraphDesc", "dagr_head_scale": "HeadScale",
            "dagr_conv_job": "ConvJob", "dagr_l0_inputs": "L0Inputs", "dagr_async_update_args": "AsyncUpdateArgs",
            "dagr_flops_module": "FlopsModule", "dagr_aug_params": "AugParams"}
    assert {c: getattr(_lib, py) for c, py in want.items()} == _lib.STRUCTS
    assert dict(_lib.AsyncUpdateArgs._fields_)["gdesc"] is POINTER(_lib.GraphDesc)
    assert dict(_lib.AsyncUpdateArgs._fields_)["pdesc"] is POINTER(_lib.PoolDesc)
    # the enumerators, and the copies that used to be written out beside them
    from dagr_amd.asynchronous import flops
    from dagr_amd.data import augment
    assert [_lib.ENUMS[k] for k in ("DAGR_OK", "DAGR_ERR_INVALID_ARG", "DAGR_ERR_HIP", "DAGR_ERR_WORKSPACE",
                                    "DAGR_ERR_UNSUPPORTED")] == [0, -1, -2, -3, -4]
    assert (flops.ZERO, flops.CONV, flops.LINEAR, flops.POOL, flops.CARTESIAN) == (0, 1, 2, 3, 4)
    assert flops.FlopsModule is _lib.FlopsModule
    dt = augment.AUG_PARAMS
    assert dt == np.dtype(_lib.AugParams) and dt.itemsize == c_layout["dagr_aug_params"] == 36
    assert {n: dt.fields[n][1] for n in dt.names} == {k.split(".")[1]: v for k, v in c_layout.items()
                                                      if k.startswith("dagr_aug_params.")}
    assert dt.names == ("flip", "crop_on", "crop_lo", "crop_hi", "zoom", "move")
    assert [dt.fields[n][0] for n in dt.names] == [np.dtype("<i4"), np.dtype("<i4"), np.dtype(("<i4", 2)),
                                                   np.dtype(("<i4", 2)), np.dtype("<f4"), np.dtype(("<i4", 2))]
