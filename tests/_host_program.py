"""One builder for the stand-alone host programs of the suite (tests/*_host.cpp: a device header of csrc behind tests/host_shim.h,
with its own main).  The program is compiled with the host compiler, by default under AddressSanitizer and UBSan with every report
fatal, and RUN AS A PROGRAM by its test: nothing is loaded into Python under a sanitizer.  No GPU involved."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
SANITIZE = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def build(name, workdir, flags=(), sanitize=True):
    """tests/<name>.cpp -> the executable <workdir>/<name> (its path).  -ffp-contract=off: an fmaf is where the source says so and
    nowhere else.  A missing compiler or a failed compile raises."""
    assert CXX, "a host C++ compiler is needed"
    exe = os.path.join(str(workdir), name)
    subprocess.check_call([CXX, "-O2", "-std=c++17", "-ffp-contract=off", *(SANITIZE if sanitize else ()), *flags, "-o", exe,
                           os.path.join(HERE, name + ".cpp")])
    return exe
