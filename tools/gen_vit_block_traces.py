"""Writes tests/golden/vit_block_traces.json: the launch trace of every case of tests/test_gpu_vit_blocks.py, recorded on the CPU
through the emulator (tests/hipemu.py) from a checkout of the commit whose block loops are the yardstick:

    git worktree add ../parent <commit>
    python tools/gen_vit_block_traces.py --package ../parent

The cases, the recorder and the emulator are this tree's; only the ``sam6d_amd`` package is the checkout's.  The file holds op
names, shapes, dtypes and flags only (no values, no time stamps): it regenerates identically on any machine."""
import argparse
import ctypes
import importlib.util
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def use_package(root):
    """``import sam6d_amd`` -> the package under `root`, whatever sys.path says."""
    pkg = os.path.join(os.path.abspath(root), "sam6d_amd")
    spec = importlib.util.spec_from_file_location("sam6d_amd", os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["sam6d_amd"] = mod
    spec.loader.exec_module(mod)


def use_emulator():
    """What the `emu` fixture of tests/conftest.py does, for a plain process."""
    import torch

    from sam6d_amd import _lib, ops
    from tests import hipemu
    L = ctypes.CDLL(hipemu.build())
    L.s6d_strerror.restype = ctypes.c_char_p
    L.s6d_strerror.argtypes = [ctypes.c_int]
    L.s6d_last_hip_error.restype = ctypes.c_char_p
    _lib._lib = L
    ops._stream = lambda: ctypes.c_void_p(0)
    torch.Tensor.is_cuda = property(lambda self: True)
    torch.Tensor.cuda = lambda self, *a, **k: self


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--package", default=ROOT, help="checkout whose sam6d_amd is recorded")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "vit_block_traces.json"))
    a = ap.parse_args()
    use_package(a.package)
    use_emulator()
    from tests import test_gpu_vit_blocks as T
    commit = subprocess.check_output(["git", "-C", a.package, "rev-parse", "HEAD"], text=True).strip()
    cases = {name: T.run_case(name, dev="cpu")[0] for name in T.CASES}
    with open(a.out, "w") as f:                                       # one launch per line
        f.write('{"commit": %s, "cases": {\n' % json.dumps(commit) + ",\n".join(
            '%s: [\n%s]' % (json.dumps(name), ",\n".join(json.dumps(e, sort_keys=True) for e in trace))
            for name, trace in cases.items()) + "}}\n")
    print(a.out, os.path.getsize(a.out), "bytes;", {k: len(v) for k, v in cases.items()})


if __name__ == "__main__":
    main()
