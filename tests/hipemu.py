"""Host build of the kernel sources against the emulated HIP runtime (tests/host_cc/hipemu): libsam6d_emu.so exports the same
C ABI as libsam6d_hip.so but takes HOST pointers and runs every launch on the CPU (lanes = fibers, wave collectives and MFMA
emulated).  TEST INFRASTRUCTURE -- slow, for small shapes; lets kernel logic be checked against the oracle without a GPU."""
import ctypes
import glob
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(REPO, "sam6d_amd", "csrc")
EMU = os.path.join(HERE, "host_cc", "hipemu")
OUT = os.path.join(HERE, "host_cc", "_build")
# HIPEMU_EXTRA: extra compiler flags (e.g. "-DS6D_RPE_FOUR_KEYS_MAX_ROWS=0" for a kernel variant, as tests/test_emu_pose.py passes);
# each setting gets its own library file
EXTRA = os.environ.get("HIPEMU_EXTRA", "").split()
SO = os.path.join(OUT, "libsam6d_emu" + ("_" + re.sub(r"[^A-Za-z0-9]+", "_", "".join(EXTRA)) if EXTRA else "") + ".so")
CXX = os.environ.get("HIPEMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")

_lib = None


def _stale():
    if not os.path.exists(SO):
        return True
    t = os.path.getmtime(SO)
    deps = glob.glob(os.path.join(CSRC, "*")) + glob.glob(os.path.join(EMU, "**", "*"), recursive=True) + [__file__]
    return any(os.path.isfile(d) and os.path.getmtime(d) > t for d in deps)


def build(force=False, files=None):
    if not force and not _stale() and files is None:
        return SO
    os.makedirs(OUT, exist_ok=True)
    srcs = []
    for f in sorted(glob.glob(os.path.join(CSRC, "*.hip"))):
        if files is not None and os.path.basename(f) not in files:
            continue
        dst = os.path.join(OUT, os.path.basename(f)[:-4] + ".cc")              # the text itself is not touched
        with open(dst, "w") as g:
            g.write(f'#line 1 "{f}"\n' + open(f).read())
        srcs.append(dst)
    cmd = [CXX, "-O2", "-std=c++17", "-fPIC", "-shared", "-w", "-ffp-contract=off"] + EXTRA + ["-I", EMU, "-I", CSRC, "-I",
           os.path.join(REPO, "include"), "-o", SO, os.path.join(EMU, "hipemu.cc")] + srcs
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        raise RuntimeError("hipemu build failed:\n" + r.stderr[-6000:])
    return SO


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build())
    return _lib


def ptr(a):
    """numpy array (C-contiguous) -> void*"""
    assert a.flags["C_CONTIGUOUS"]
    return ctypes.c_void_p(a.ctypes.data)
