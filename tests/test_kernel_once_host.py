"""The native library's "once per kernel" helper (csrc/kernel_once.h) under ThreadSanitizer, on the host: a stand-alone program
with a counting setter (tests/host_cpp/kernel_once_main.cpp), built with the system C++ compiler and run as a process of its own."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_kernel_once_helper_under_thread_sanitizer(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no system C++ compiler")
    exe = str(tmp_path / "kernel_once_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=thread", "-pthread", os.path.join(HERE, "host_cpp", "kernel_once_main.cpp"),
                    "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)   # (the program carries its sanitizer runtime itself)
    assert r.returncode == 0 and "kernel_once: ok" in r.stdout and "ThreadSanitizer" not in r.stderr, r.stdout + r.stderr
