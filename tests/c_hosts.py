"""How the tests build the C hosts of examples/: with hipcc, against include/marigold_hip.h and the in-tree libmarigold_hip.so - what a
host without Python does.  One copy of the command for every test that runs or compiles an example."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
INCLUDE, LIB_DIR = os.path.join(ROOT, "include"), os.path.join(ROOT, "marigold_amd")


def have_hipcc():
    return os.path.exists(HIPCC)


def _hipcc(args, why):
    assert have_hipcc(), f"hipcc is needed to {why}"
    r = subprocess.run([HIPCC] + args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]


def build_example(name, dest_dir):
    """examples/``name``.cpp compiled and linked against the in-tree library (found at run time by its rpath) -> the program's path in
    ``dest_dir``."""
    exe = os.path.join(str(dest_dir), name)
    _hipcc(["-O2", os.path.join(ROOT, "examples", name + ".cpp"), "-I" + INCLUDE, "-L" + LIB_DIR, "-lmarigold_hip", "-Wl,-rpath," + LIB_DIR, "-o", exe],
           "build the C host")
    return exe


def compile_only(path, out):
    """The header checks: ``path`` compiled against include/marigold_hip.h, nothing linked from the library - to the program ``out``, or,
    for an ``out`` that ends in .o, to the gfx950 object of an example."""
    path, out = str(path), str(out)
    mode = ["-O2", "--offload-arch=gfx950", "-c"] if out.endswith(".o") else ["-x", "c++"]
    _hipcc(mode + [path, "-I" + INCLUDE, "-o", out], "compile against the header")
    return out
