"""The C-ABI library builds, loads without a GPU and exports exactly what include/grit_hip.h declares; the binding is that header, read
by grit_amd/abi.py: its struct layouts are checked against the C compiler, its type mapping against prototypes written out by hand,
and the reader refuses what it does not fully understand."""
import ctypes
import os
import re
import subprocess

import pytest

from grit_amd import abi, build, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I, L, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float
I64, U64 = ctypes.c_int64, ctypes.c_uint64


def _declared():
    text = open(os.path.join(ROOT, "include", "grit_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(grit_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_exported_and_bound():
    build.build_hip()
    names = _declared()
    assert "grit_msda_fwd_f32" in names and "grit_msda_bwd_f32" in names
    dll = ctypes.CDLL(lib.LIB_PATH)
    for n in names:
        assert hasattr(dll, n), "missing export " + n
    assert sorted(lib.SIGNATURES) == names, "the reader and a plain search for `grit_xxx(` disagree on what the header declares"
    assert len(names) >= 85


def test_struct_layouts_match_the_c_compiler(tmp_path):
    """sizeof and every offsetof of the header's structs, from gcc, against the generated ctypes classes."""
    structs = abi.read().structs
    assert len(structs) >= 9
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "grit_hip.h"', 'int main(void) {']
    for name, fields in structs.items():
        lines.append('    printf("%s sizeof %%zu\\n", sizeof(%s));' % (name, name))
        lines += ['    printf("%s %s %%zu\\n", offsetof(%s, %s));' % (name, f, name, f) for f, _ in fields]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines + ["    return 0;", "}", ""]))
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    from_c = [tuple(line.split()) for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()]
    from_ctypes = []
    for name, fields in structs.items():
        cls = getattr(lib, "".join(w.capitalize() for w in name[len("grit_"):].split("_")))
        assert [f for f, _ in cls._fields_] == [f for f, _ in fields]
        from_ctypes.append((name, "sizeof", str(ctypes.sizeof(cls))))
        from_ctypes += [(name, f, str(getattr(cls, f).offset)) for f, _ in fields]
    assert from_ctypes == from_c
    assert {"WgradJob", "RelbiasBwdJob", "NormRange", "CiderTables", "ScoreTables", "SlabJob", "ColsumJob", "RelbiasJob",
            "TransposeJob"} <= set(vars(lib))
    assert lib.CiderTables.idf_start.size == 5 * ctypes.sizeof(L) and ctypes.sizeof(lib.WgradJob) == 80


def test_type_mapping_of_pinned_prototypes():
    """Written out by hand from the header, one prototype per scalar type; pointers of every kind are c_void_p."""
    functions = abi.read().functions
    assert functions["grit_wgrad_tn"] == (I, [P, L, P, L, I, I, I, I, P, P, P])
    attn_in = [P, I64, I64] * 4  # q, k, v, mask, each with two int64_t strides
    assert functions["grit_attn_fwd_f32"] == (I, attn_in + [I] * 5 + [F, F, U64, P, P, P, P])
    assert functions["grit_winattn_fwd_bf16"] == (I, [P] * 4 + [I] * 8 + [F, P, P, P])
    assert functions["grit_adam_flat"][1][6:14] == [L] + [F] * 7
    assert functions["grit_status_string"] == (ctypes.c_char_p, [I])
    assert functions["grit_beam_step_workspace"] == (L, [I, I, I])
    assert functions["grit_abi_version"] == (I, [])
    assert functions["grit_beam_step"] == (I, [P, P])  # the argument struct and the stream
    assert not {"grit_beam_step_f32", "grit_beam_step_mean_f32", "grit_beam_step_con_f32", "grit_beam_step_div_f32",
                "grit_beam_step_forced_f32"} & set(functions)
    assert abi.read().structs["grit_beam_step_args"] == [
        ("maps", P), ("n_maps", I), ("ld", L),
        ("seq_logprob", P), ("seq_mask", P), ("prev_words", P), ("eos", I), ("first_step", I),
        ("B", I), ("cur_beam", I), ("V", I), ("k", I),
        ("history", P), ("history_ld", L), ("t", I), ("no_repeat_ngram", I), ("no_repeat_word", I), ("ban_eos", I), ("suppress", P),
        ("n_suppress", I),
        ("groups", I), ("diversity", F),
        ("force_words", P), ("n_sets", I), ("n_words", I), ("met_in", P),
        ("workspace", P), ("workspace_bytes", L),
        ("sel_beam", P), ("sel_word", P), ("new_seq_logprob", P), ("new_seq_mask", P), ("picked_logprob", P), ("new_met", P)]
    assert lib.SIGNATURES["grit_wgrad_tn"] == functions["grit_wgrad_tn"][1]
    loaded = lib.load()
    assert loaded.grit_beam_step_workspace.restype is L and loaded.grit_status_string.restype is ctypes.c_char_p
    assert loaded.grit_attn_fwd_f32.argtypes == functions["grit_attn_fwd_f32"][1]
    fields = dict(abi.read().structs["grit_cider_tables"])
    assert fields["idf_start"]._length_ == 5 and fields["idf_start"]._type_ is L and fields["sigma"] is ctypes.c_double


def test_constants_come_from_the_header():
    constants = abi.read().constants
    assert constants["GRIT_ABI_VERSION"] == abi.read().version == lib.ABI_VERSION
    assert (lib.OK, lib.ERR_BAD_ARG, lib.ERR_UNSUPPORTED, lib.ERR_LAUNCH) == (0, 1, 2, 3)
    assert (lib.SLAB_GROUP_MAX, lib.LN_BWD_PARTIALS, lib.GEMM_BIAS_GELU, lib.GEMM_COLSUM_ROWS, lib.AUG_SHARPNESS) == (48, 1024, 2, 128, 7)
    assert "GRIT_IMAGE_TMP_PITCH" not in constants and "GRIT_HIP_H" not in constants  # a macro with arguments, the include guard
    for name, value in constants.items():
        assert getattr(lib, name[len("GRIT_"):]) == value


GOOD = """
#ifndef X_H
#define X_H
#define GRIT_A 3   /* three */
#define GRIT_HEX 0x10
#define GRIT_PITCH(w) ((w) + 3)
typedef struct grit_t {
    const void* p; long n;
    int a, b;          // two fields
    double d[5];
    const float* const* rows;
} grit_t;
int grit_none(void);
const char* grit_text(int status);
long grit_f(const grit_t* jobs, /* between */ const float x[], int const n, unsigned long long u,
            double const* const w, void* stream);
#endif
"""


def test_reader_accepts_the_subset():
    got = abi.parse(GOOD)
    assert got.constants == {"GRIT_A": 3, "GRIT_HEX": 16} and got.version is None
    assert got.structs == {"grit_t": [("p", P), ("n", L), ("a", I), ("b", I), ("d", ctypes.c_double * 5), ("rows", P)]}
    assert got.functions == {"grit_none": (I, []), "grit_text": (ctypes.c_char_p, [I]),
                             "grit_f": (L, [P, P, I, ctypes.c_ulonglong, P, P])}


@pytest.mark.parametrize("snippet, named", [
    ("int grit_f(short x);", "grit_f(short x)"),                                    # a type outside the list
    ("int grit_f(int n, size_t* p);", "size_t"),                                    # ... also behind a pointer
    ("int grit_f(int (*callback)(int), void* stream);", "grit_f"),                  # function-pointer parameter
    ("int grit_f(int a, int b)\nint grit_g(void);", "grit_f(int a, int b) int grit_g"),  # unterminated prototype
    ("int grit_g(void);\nint grit_f(int a,", "grit_f(int a,"),                      # ... at the end of the file
    ("int grit_f(int);", "grit_f(int)"),                                            # unnamed parameter
    ("typedef struct { int a; struct { int b; } in; } grit_t;", "struct { int b"),  # nested struct
    ("typedef struct { int a; short b; } grit_t;", "short b"),
    ("typedef struct { float *a, *b; } grit_t;", "float *a, *b"),
    ("typedef int grit_status;", "typedef int grit_status"),
    ("#define GRIT_N (1 << 4)\n", "GRIT_N"),                                        # not a plain integer
    ("#if defined(X)\n#endif\n", "#if defined(X)"),
])
def test_reader_refuses_what_it_cannot_parse(snippet, named):
    with pytest.raises(abi.AbiError) as err:
        abi.parse(snippet)
    assert named in str(err.value)


def test_load_and_status_strings():
    l = lib.load()
    assert l.grit_abi_version() == lib.ABI_VERSION
    assert l.grit_status_string(0) == b"ok"
    assert b"launch" in l.grit_status_string(3)


def test_header_cites_reference_interfaces():
    text = open(os.path.join(ROOT, "include", "grit_hip.h")).read()
    for cite in ("ms_deform_attn.h:20", "vision.cpp", "swin_model.py:155", "attention.py:51"):
        assert cite in text


def test_cpu_tensors_are_rejected_like_the_reference():
    import pytest
    import torch
    from grit_amd.ops.msda import ms_deform_attn_forward
    shapes = torch.tensor([[2, 2]]); lsi = torch.tensor([0])
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ms_deform_attn_forward(torch.zeros(1, 4, 1, 4), shapes, lsi, torch.zeros(1, 1, 1, 1, 1, 2),
                               torch.zeros(1, 1, 1, 1, 1))


def test_one_hip_runtime_whatever_is_loaded_first():
    """libgrit_hip.so loaded BEFORE torch must end up on torch's HIP runtime (two runtimes in one process do not share streams):
    the library finds `libamdhip64.so.7` next to itself, a link to torch's copy made by the build."""
    import subprocess
    import sys
    from grit_amd import lib
    code = (
        "import ctypes\n"
        "l = ctypes.CDLL(%r)\n"
        "assert l.grit_abi_version() == %d\n"
        "import torch, os\n"
        "maps = open('/proc/self/maps').read()\n"
        "libs = sorted({x.split()[-1] for x in maps.split('\\n') if 'libamdhip64' in x})\n"
        "print(len(libs), os.path.realpath(libs[0]).startswith(os.path.dirname(torch.__file__)))\n" % (lib.LIB_PATH, lib.ABI_VERSION))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["1", "True"], out.stdout
