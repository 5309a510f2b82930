"""CPU: the ctypes side of the C ABI is read from include/ptv2_hip.h (ao_amd/_abi.py), not written by hand.

1. The derived tables equal tests/golden/abi_parent.json, recorded from the hand-written tables of the commit before the
   reader existed (profiles/HISTORY.md has the recipe): every function's result and argument types, every struct's size
   and [field, offset, size] rows, the constants the python side used.  One mapping is allowed: the three host-only calls
   that were typed POINTER(x) are c_void_p now (their callers pass byref() / ctypes arrays, which c_void_p accepts).
2. The derived struct layouts equal what the host C compiler makes of the header: sizeof of every struct, offsetof and size
   of every field -- the compiler the library's structs come from, field by field.
3. The reader raises on what it cannot map, naming the declaration, and reads the forms the header uses.
"""
import ctypes
import json
import os
import shutil
import subprocess

import pytest

from tests.conftest import GOLDEN, ROOT

POINTER_TYPED_BEFORE = ("ptv2_profile_read", "ptv2_graph_stats", "ptv2_gva_plan_describe")


@pytest.fixture(scope="module")
def abi():
    from ao_amd import _abi

    return _abi


def layout(cls):
    return {"size": ctypes.sizeof(cls),
            "fields": [[f[0], getattr(cls, f[0]).offset, getattr(cls, f[0]).size] for f in cls._fields_]}


def test_derived_tables_equal_the_hand_written_ones_of_the_parent(abi):
    with open(os.path.join(GOLDEN, "abi_parent.json")) as f:
        parent = json.load(f)
    assert len(parent["functions"]) == 127 and len(parent["structs"]) == 13
    assert sorted(abi.signatures) == sorted(parent["functions"])
    remapped = set()
    for name, (res, args) in parent["functions"].items():
        have_res, have_args = abi.signatures[name]
        want = [res] + args
        if any(t.startswith("POINTER(") for t in want):
            assert name in POINTER_TYPED_BEFORE, name
            remapped.add(name)
            want = ["c_void_p" if t.startswith("POINTER(") else t for t in want]
        assert [have_res.__name__] + [t.__name__ for t in have_args] == want, name
    assert remapped == set(POINTER_TYPED_BEFORE)
    assert list(abi.structs) == ["ptv2_gva_block", "ptv2_gva_block_grads", "ptv2_inverse_job", "ptv2_block", "ptv2_block_grads",
                                 "ptv2_linbn", "ptv2_level", "ptv2_seq", "ptv2_model_block", "ptv2_model", "ptv2_geo_table",
                                 "ptv2_geo_level", "ptv2_scene_geo"]  # header order
    assert {name: layout(cls) for name, cls in abi.structs.items()} == parent["structs"]
    assert ctypes.sizeof(abi.structs["ptv2_model"]) == 29512 and ctypes.sizeof(abi.structs["ptv2_scene_geo"]) == 1144
    assert {name: abi.consts[name] for name in parent["constants"]} == parent["constants"]
    assert len(abi.consts) == 40 and abi.consts["PTV2_BLK_FC1_W"] == 0 and abi.consts["PTV2_BLK_N3_B"] == 29


def test_the_python_side_uses_the_derived_tables(abi):
    from ao_amd import _lib
    from ao_amd.ptv2 import block, geometry, gva, native_model

    assert _lib._SIGNATURES is abi.signatures
    S = abi.structs
    assert (gva._BlockArgs, gva._BlockGrads, gva._InverseJob) == (S["ptv2_gva_block"], S["ptv2_gva_block_grads"], S["ptv2_inverse_job"])
    assert (block._Blk, block._BlkGrads) == (S["ptv2_block"], S["ptv2_block_grads"])
    assert (native_model._LinBn, native_model._Level, native_model._Seq, native_model._MBlock, native_model._Model) == (
        S["ptv2_linbn"], S["ptv2_level"], S["ptv2_seq"], S["ptv2_model_block"], S["ptv2_model"])
    assert (geometry._GeoTable, geometry._GeoLevel, geometry._SceneGeo) == (S["ptv2_geo_table"], S["ptv2_geo_level"], S["ptv2_scene_geo"])
    assert (block.NPARAM, block.NBN, native_model.MAX_STAGES, native_model.MAX_BLOCKS, geometry._MAX_STAGES, geometry._GEO_MAX_K,
            gva.INVERSE_MAX_JOBS) == (30, 7, 5, 40, 5, 2, 16)
    L = _lib.lib()
    for name, (res, args) in abi.signatures.items():  # lib() has bound every derived entry
        assert getattr(L, name).restype is res and getattr(L, name).argtypes == args, name
    assert L.ptv2_struct_bytes(4) == ctypes.sizeof(geometry._SceneGeo)


def host_compiler():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    return (shutil.which("cc") or shutil.which("gcc") or shutil.which("clang", path=os.path.join(rocm, "llvm", "bin"))
            or shutil.which("clang", path=os.path.join(rocm, "lib", "llvm", "bin")))


def test_struct_layouts_equal_the_c_compilers(abi, tmp_path):
    cc = host_compiler()
    if cc is None:
        pytest.skip("no host C compiler (cc, gcc, ROCm's clang)")
    lines = ["#include <stdio.h>", '#include "ptv2_hip.h"', "int main(void) {"]
    for name, cls in abi.structs.items():
        lines.append('    printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        for f in cls._fields_:
            lines.append('    printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));'
                         % (name, f[0], name, f[0], name, f[0]))
    lines += ["    return 0;", "}", ""]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    have = {}
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        key, *numbers = line.split()
        have[key] = [int(n) for n in numbers]
    want = {}
    for name, cls in abi.structs.items():
        want[name] = [ctypes.sizeof(cls)]
        for f in cls._fields_:
            want["%s.%s" % (name, f[0])] = [getattr(cls, f[0]).offset, getattr(cls, f[0]).size]
    assert len(want) == 13 + sum(len(cls._fields_) for cls in abi.structs.values()) and len(want) > 200
    assert have == want


def test_reader_reads_the_forms_the_header_uses(abi):
    consts, structs, signatures = abi.parse("""
        #define N 3
        enum { A, B = 2 * N, C, D = A + 1, E };
        typedef struct inner { const int *a, b, *c; volatile unsigned u; } inner;
        typedef struct outer { inner one, many[N + 1]; const float *const *pp; double d[2 * N]; char *s; long long q; } outer;
        const char *name_of(const outer *o, size_t n, char *buf, const char *const *list, float w[4], unsigned long long *k);
        long long count(void);
    """)
    assert consts == {"N": 3, "A": 0, "B": 6, "C": 7, "D": 1, "E": 2}
    inner, outer = structs["inner"], structs["outer"]
    assert [t for _, t in inner._fields_] == [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint]
    fields = dict(outer._fields_)
    assert fields["one"] is inner and fields["many"]._type_ is inner and fields["many"]._length_ == 4
    assert fields["pp"] is ctypes.c_void_p and fields["d"]._type_ is ctypes.c_double and fields["d"]._length_ == 6
    assert fields["s"] is ctypes.c_char_p and fields["q"] is ctypes.c_longlong
    assert signatures == {"name_of": (ctypes.c_char_p, [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_void_p,
                                                        ctypes.c_void_p, ctypes.c_void_p]),
                          "count": (ctypes.c_longlong, [])}


@pytest.mark.parametrize("text, names", [
    ("typedef struct s { int n; half *x; } s;", ("struct s", "half")),              # unknown type in a field
    ("typedef struct s { short n; } s;", ("struct s", "short")),
    ("int f(int n, const half *x, void *stream);", ("f", "half")),                   # unknown type in a parameter
    ("int f(long n);", ("f", "long")),
    ("typedef struct s { float *p[UNDEFINED + 1]; } s;", ("struct s", "UNDEFINED")),  # array bound of an undefined constant
    ("#define N M", ("N", "M")),
    ("typedef struct s { struct { int a; } in; } s;", ("struct",)),                  # outside the subset: not skipped
    ("int f(int (*callback)(int));", ("callback",)),
    ("int f(int n);\nstatic inline int g(void) { return 1; }\nint h(void);", ("static inline",)),
    ("#if 0\nint f(int n);\n#endif", ("#if 0",)),
])
def test_reader_refuses_what_it_does_not_understand(abi, text, names):
    with pytest.raises(RuntimeError) as err:
        abi.parse(text)
    for name in names:
        assert name in str(err.value), str(err.value)
