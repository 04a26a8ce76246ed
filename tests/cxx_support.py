"""Shared by the tests that drive a C++ program of tests/cxx/ over stdin / stdout (test_cxx_learner, test_device_learner): build it,
format its input, read its lines.  No test imports a test."""
import os
import subprocess

import numpy as np

from conftest import ROOT

BUILD = os.path.join(ROOT, "build")


def _cxx(name, hip_built=None, extra=(), out=None):
    """g++ tests/cxx/<name>.cpp (+ `extra` sources / flags) -> build/<out or name>; linked with libmoihgp when `hip_built` is its path."""
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, out or name)
    cmd = ["g++", "-std=c++14", "-O1", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cxx"),
           os.path.join(ROOT, "tests", "cxx", name + ".cpp"), *extra, "-o", exe]
    if hip_built:
        libdir = os.path.dirname(hip_built)
        cmd += ["-L", libdir, "-lmoihgp", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.run(cmd, check=True)
    return exe


def _fmt(a):
    return " ".join(repr(float(v)) for v in np.asarray(a, dtype=np.float64).ravel())


def _lines(exe, inp):
    return subprocess.run([exe], input=inp, capture_output=True, text=True, check=True).stdout.strip().split("\n")


def _arr(line):
    return np.array(line.split(), dtype=float)
