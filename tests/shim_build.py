"""The one way the tests build a tests/shim_*.cpp program: against the stand-in PCL / Eigen headers of tests/standins, the shim headers and include/qn_engine.h,
linked with the in-tree libqn_engine.so (found at run time through an rpath)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_shim(source_name, out_dir, *more_sources, link=True):
    """tests/<source_name> (a source elsewhere: its absolute path) and more_sources, further translation units of the same program -> the path of the program,
    out_dir/<the first source's name without .cpp>.  link=False: a program that must do without the library."""
    from qn_amd import build
    build.build()
    pkg = os.path.join(ROOT, "fast-lio-sam-qn_amd")
    exe = os.path.join(str(out_dir), os.path.splitext(os.path.basename(source_name))[0])
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "tests", "standins"), "-I" + os.path.join(pkg, "shim"),
                           "-I" + os.path.join(ROOT, "include")] + [os.path.join(ROOT, "tests", s) for s in (source_name,) + more_sources] +
                          (["-L" + pkg, "-lqn_engine", "-Wl,-rpath," + pkg] if link else []) + ["-o", exe])
    return exe
