"""The C-ABI library loads on a CPU-only host and exports every symbol include/sam6d_hip.h declares
(no compute calls: there is no GPU here)."""
import ctypes

from sam6d_amd import _lib


def test_library_loads_and_exports_every_declared_symbol():
    L = _lib.lib()
    names = _lib.declared_symbols()
    assert len(names) >= 25
    missing = [n for n in names if not hasattr(L, n)]
    assert not missing, missing
    assert L.s6d_version() >= 100
    assert L.s6d_strerror(-1).decode().startswith("invalid argument")


def test_argument_validation_without_a_gpu():
    """Entry points validate sizes/pointers before touching the device: callable on a CPU-only host."""
    L = _lib.lib()
    assert L.s6d_fps_f32(None, 1, 0, 1, None, None, None) == -1          # N <= 0
    assert L.s6d_fps_f32(None, 0, 10, 4, None, None, None) == 0           # B == 0: nothing to do
    assert L.s6d_fps_f32(None, 1, 10, 4, None, None, None) == -1          # null pointers
    assert L.s6d_rpe_attention_f32(None, None, None, None, None, None, 1, 197, 128, 4, ctypes.c_float(1.0), None, None) == -3


def test_round3_entry_points_validate_shapes_without_a_gpu():
    """The folded-GEMM, statistics and linear-attention entries reject what they do not implement before any launch (fake non-null
    pointers: nothing is dereferenced on these paths)."""
    L = _lib.lib()
    p = ctypes.c_void_p(4096)
    lng, flt = ctypes.c_long, ctypes.c_float
    # N % 256 != 0: the 256 x 256-tile kernel only
    assert L.s6d_gemm_bf16_lnfold(p, lng(64), p, p, lng(64), p, p, p, lng(128), 256, 128, 64, 0, 0, 0, None) == -3
    assert L.s6d_gemm_bf16_lnfold(p, lng(64), p, p, lng(64), p, p, p, lng(256), 256, 256, 64, 2, 0, 0, None) == -1       # gelu flag
    assert L.s6d_gemm_bf16_res(p, lng(64), p, lng(64), p, p, lng(128), None, p, lng(128), 256, 128, 64, 0, None) == -3
    assert L.s6d_gemm_bf16_res(p, lng(64), p, lng(64), p, p, lng(100), None, p, lng(256), 256, 256, 64, 0, None) == -1     # ldr < N
    assert L.s6d_ln_stats_finalize(p, 0, 32, lng(16), flt(1e-6), p, None) == -1
    assert L.s6d_ln_stats_finalize(p, 40, 32, lng(0), flt(1e-6), p, None) == 0                                               # no rows
    assert L.s6d_row_stats_bf16(p, lng(1284), lng(4), 1284, flt(1e-6), p, None) == -1                                        # C % 8
    assert L.s6d_row_stats_bf16(p, lng(2048), lng(4), 2048, flt(1e-6), p, None) == -3                                        # C > 1536
    assert L.s6d_linear_attention_f32(p, p, 3, p, lng(128), p, lng(128), 1, 8, 8, 128, p, p, None) == -3                     # C != 256
    assert L.s6d_linear_attention_f32(p, p, 3, p, lng(100), p, lng(256), 1, 8, 8, 256, p, p, None) == -1                     # ldk < C
    assert L.s6d_rpe_attention_strided_f32(p, lng(258), p, lng(256), p, lng(256), p, p, p, 1, 8, 256, 4, flt(1.0), p, None) == -1   # ld % 4
    assert L.s6d_mha_strided_f32(p, lng(768), p, lng(512), p, lng(512), 0, 8, 8, 256, 4, flt(1.0), p, None) == 0             # B == 0


def test_ops_refuse_cpu_tensors():
    import pytest
    import torch
    from sam6d_amd import ops
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ops.ball_query(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3), 0.1, 4)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        ops.rpe_attention(*([torch.zeros(1, 4, 256)] * 3), torch.zeros(1, 4, 4, 256), torch.zeros(1, 4, 4),
                          torch.zeros(1, 4, 4, 256), 0.125)


def test_every_entry_point_refuses_null_operands():
    """Generated from the header (_lib.prototypes()): each `int s6d_*(...)` entry point with a pointer parameter is called with
    NULL for every pointer and small positive sizes.  Every one must come back with S6D_EINVAL / S6D_EUNSUPPORTED before anything
    is dereferenced or launched (this host has no device, so a launch attempt would surface as S6D_ELAUNCH = -2)."""
    L = _lib.lib()
    vals = {ctypes.c_void_p: None, ctypes.c_float: 1.0, ctypes.c_double: 1.0, ctypes.c_long: 16, ctypes.c_int: 16}
    # (no pointer = no operand to refuse: s6d_version, the s6d_set_* switches, the workspace sizes)
    protos = {n: a for n, (r, a) in _lib.prototypes().items() if r is ctypes.c_int and ctypes.c_void_p in a}
    assert len(protos) == len(_lib.declared_symbols()) - sum(r is not ctypes.c_int or ctypes.c_void_p not in a
                                                             for r, a in _lib.prototypes().values()) >= 28
    rcs = {name: getattr(L, name)(*[vals[t] for t in args]) for name, args in protos.items()}
    assert all(rc in (-1, -3) for rc in rcs.values()), rcs


def test_header_is_the_prototype_table():
    """Every declared entry point has a prototype, the loaded library carries it, and a type the parser does not know is an error
    that names the prototype (a header string with one injected declaration; the header itself is not touched)."""
    import os

    import pytest
    protos = _lib.prototypes()
    assert sorted(protos) == _lib.declared_symbols() and len(protos) >= 25
    assert {r for r, _ in protos.values()} == {ctypes.c_int, ctypes.c_long, ctypes.c_char_p}
    assert {t for _, a in protos.values() for t in a} == {ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float}
    assert protos["s6d_fps_f32"] == (ctypes.c_int, (ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int) + (ctypes.c_void_p,) * 3)
    assert protos["s6d_version"] == (ctypes.c_int, ()) and protos["s6d_strerror"] == (ctypes.c_char_p, (ctypes.c_int,))
    assert protos["s6d_nms_workspace_bytes"] == (ctypes.c_long, (ctypes.c_int,))
    L = _lib.lib()
    for name, (restype, argtypes) in protos.items():
        assert getattr(L, name).restype is restype and tuple(getattr(L, name).argtypes) == argtypes, name
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "sam6d_hip.h")).read()
    assert _lib.parse_header(hdr) == (_lib.abi_version(), protos)
    for decl in ("int s6d_new_thing(const float *x, size_t n, void *stream);", "int64_t s6d_new_thing(const float *x);",
                 "int s6d_new_thing(unsigned int n);"):
        with pytest.raises(ValueError, match="s6d_new_thing"):
            _lib.parse_header(hdr.replace("int s6d_version(void);", decl + "\nint s6d_version(void);"))
    _, more = _lib.parse_header(hdr.replace("int s6d_version(void);", "long s6d_new_thing(const double *const x, double y, const int n);\n"
                                                                      "int s6d_version(void);"))
    assert more["s6d_new_thing"] == (ctypes.c_long, (ctypes.c_void_p, ctypes.c_double, ctypes.c_int)) and len(more) == len(protos) + 1


def test_ops_name_only_declared_entry_points():
    """Static: every string literal beginning `s6d_` that reaches _call / _size in sam6d_amd/ops.py, and every value of the have()
    map, is a declared entry point -- or, where the name is finished at run time ("s6d_seq_attention_" + suffix), a prefix of one."""
    import ast
    import os

    from sam6d_amd import ops
    declared = _lib.declared_symbols()
    tree = ast.parse(open(os.path.splitext(ops.__file__)[0] + ".py").read())
    names, prefixes = set(), set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and getattr(node.func, "id", None) in ("_call", "_size"):
            lits = [c.value for c in ast.walk(node.args[0]) if isinstance(c, ast.Constant) and isinstance(c.value, str)]
            assert lits and all(v.startswith("s6d_") for v in lits), (node.lineno, lits)
            (prefixes if isinstance(node.args[0], ast.BinOp) else names).update(lits)
        if isinstance(node, ast.FunctionDef) and node.name == "have":
            maps = [d for d in ast.walk(node) if isinstance(d, ast.Dict)]
            assert len(maps) == 1 and len(maps[0].values) >= 40
            names.update(v.value for v in maps[0].values)
    assert len(names) >= 70 and prefixes
    assert not [n for n in names if n not in declared], [n for n in names if n not in declared]
    assert all(any(d.startswith(p) and d != p for d in declared) for p in prefixes), prefixes
    every = {c.value for c in ast.walk(tree) if isinstance(c, ast.Constant) and isinstance(c.value, str) and c.value.startswith("s6d_")}
    assert every == names | prefixes, every - names - prefixes          # no entry-point name goes to the library by another road


def test_calls_are_checked_against_the_prototype():
    """One argument too many or too few is a TypeError, a float where a pointer or an int is declared a ctypes.ArgumentError, an
    unknown name an AttributeError: all before the library is entered (s6d_fps_f32 with B = 0 is otherwise a no-op returning 0)."""
    import pytest

    from sam6d_amd import ops
    args = (None, 0, 10, 4, None, None, None)
    ops._call("s6d_fps_f32", *args)
    with pytest.raises(TypeError, match="s6d_fps_f32 takes 7 arguments"):
        ops._call("s6d_fps_f32", *args, None)
    with pytest.raises(TypeError, match="s6d_fps_f32 takes 7 arguments"):
        ops._call("s6d_fps_f32", *args[:-1])
    with pytest.raises(TypeError):
        _lib.lib().s6d_fps_f32(*args[:-1])                     # (too few: ctypes' own check on the typed function)
    for bad in ((1.5,) + args[1:], args[:1] + (0.0,) + args[2:], args[:3] + (4.0,) + args[4:]):
        with pytest.raises(ctypes.ArgumentError):
            ops._call("s6d_fps_f32", *bad)
    with pytest.raises(AttributeError, match="s6d_no_such_entry"):
        ops._call("s6d_no_such_entry", None)
    with pytest.raises(_lib.S6DError, match="s6d_fps_f32"):
        ops._call("s6d_fps_f32", None, 1, 0, 1, None, None, None)          # N <= 0: the code still goes through _lib.check
    assert ops._size("s6d_nms_workspace_bytes", 100000) > 2 ** 30          # a `long` result comes back whole
    with pytest.raises(TypeError, match="s6d_nms_workspace_bytes takes 1 arguments"):
        ops._size("s6d_nms_workspace_bytes", 1, 2)


def test_product_library_carries_no_emulator_code():
    """The kernel sources have `#ifdef HIPEMU` blocks for the host emulator (tests/host_cc/hipemu).  HIPEMU is defined by that
    emulator's stand-in <hip/hip_runtime.h> only, so the product build cannot see those branches: the hipcc preprocessor does not
    define it for gfx950, and libsam6d_hip.so contains neither the emulator's namespace nor its abort messages."""
    import os
    import subprocess

    from sam6d_amd import _lib
    if os.path.exists(_lib.HIPCC):
        out = subprocess.run([_lib.HIPCC, f"--offload-arch={_lib.ARCH}", "-dM", "-E", "-x", "hip", "/dev/null"], capture_output=True,
                             text=True).stdout
        assert "__gfx950__" in out and "HIPEMU" not in out
    blob = open(_lib.SO_PATH, "rb").read()
    assert b"hipemu" not in blob and b"HIPEMU" not in blob


def test_gemm4_compiler_code_leaves_the_accumulator_file_alone(tmp_path):
    """csrc/s6d_gemm4.hip keeps its 256 accumulators in a[0:255] across inline-asm blocks the compiler knows nothing about: that is
    sound only while the compiler-generated code around the blocks never touches the accumulator file and never spills.  Checked on
    the generated assembly of every instantiation: outside ;;#ASMSTART / ;;#ASMEND no instruction names an a-register, there is no
    scratch access, and the kernel descriptors reserve the whole accumulator file behind the architected registers."""
    import os
    import re
    import subprocess
    src = os.path.join(os.path.dirname(_lib.__file__), "csrc", "s6d_gemm4.hip")
    out = tmp_path / "g4.s"
    flags = [f for f in _lib.FLAGS if f not in ("-shared", "-fPIC")] + _lib.file_flags(src)
    subprocess.check_call([_lib.HIPCC] + flags + ["-S", "--cuda-device-only", "-o", str(out), src], cwd=os.path.dirname(src))
    text = out.read_text()
    kernels = re.findall(r"^(_ZN3s6d\w*gemm4_\w+):[^\n]*\n(.*?)s_endpgm", text, flags=re.M | re.S)
    assert len(kernels) >= 10
    for name, body in kernels:
        inside = False
        for line in body.splitlines():
            if "#ASMSTART" in line:
                inside = True
            elif "#ASMEND" in line:
                inside = False
            elif not inside and not line.strip().startswith(";"):
                assert not re.search(r"\ba\[?\d+|accvgpr", line), f"{name}: compiler code touches the accumulator file: {line.strip()}"
                assert "scratch_" not in line, f"{name}: spill: {line.strip()}"
    for m in re.finditer(r"\.amdhsa_kernel (\S*gemm4\S*)(.*?)\.end_amdhsa_kernel", text, flags=re.S):
        nxt = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", m.group(2)).group(1))
        off = int(re.search(r"\.amdhsa_accum_offset (\d+)", m.group(2)).group(1))
        assert nxt - off == 256 and nxt <= 512, (m.group(1), nxt, off)
