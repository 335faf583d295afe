"""The C ABI of the pose spread is additive: the header still compiles on its own as C99 and as C++ with the new declarations used
with their documented types, a C host links against them with the library alone, the version stays 5 and slam_pf_config keeps its
size; the ctypes table binds both new symbols and the Python layer has its two methods.  Needs no GPU."""
import ctypes as C
import subprocess

from __graft_entry__ import load_package

NEW = ("slam_pf_spread", "slam_pose_spread_dev")

PROGRAM = r'''
#include "%s"
static int (*const p_spread)(slam_pf *, float, float[3], float[6], float *) = slam_pf_spread;
static int (*const p_dev)(slam_engine *, const float *, const float *, const float *, const int32_t *, const float *, int, float,
                          float[3], float[6], float *) = slam_pose_spread_dev;
int main(void)
{
    float pose[3], cov[6], r;
    /* null handles are refused, not dereferenced: no GPU is touched */
    if (p_spread(0, 0.0f, pose, cov, &r) == SLAM_OK || p_dev(0, 0, 0, 0, 0, 0, 1, 0.0f, pose, cov, &r) == SLAM_OK) return 2;
    return slam_abi_version() == SLAM_ABI_VERSION && SLAM_ABI_VERSION == 5 && sizeof(slam_pf_config) == %d ? 0 : 1;
}
'''


def test_header_compiles_and_links_with_the_new_declarations(tmp_path):
    pkg = load_package()
    c = tmp_path / "t.c"
    c.write_text(PROGRAM % (pkg.HEADER_PATH, C.sizeof(pkg.PfConfig)))
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", str(c)], check=True)
    subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c++", str(c)], check=True)
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(c), f"-L{pkg.LIB_PATH.parent}", "-lslam_hip", f"-Wl,-rpath,{pkg.LIB_PATH.parent}"],
                   check=True)
    assert subprocess.run([str(exe)]).returncode == 0


def test_version_and_bindings():
    pkg = load_package()
    lib = pkg.load_library()
    assert lib.slam_abi_version() == 5
    for name in NEW:
        assert name in pkg.SIGNATURES and getattr(lib, name).argtypes == pkg.SIGNATURES[name][1]
    assert len(pkg.SIGNATURES["slam_pf_spread"][1]) == 5 and len(pkg.SIGNATURES["slam_pose_spread_dev"][1]) == 11
    assert callable(pkg.PfSession.spread) and callable(pkg.Engine.pose_spread_dev)
    text = pkg.HEADER_PATH.read_text()
    assert "#define SLAM_ABI_VERSION 5" in text and all(name + "(" in text for name in NEW)
