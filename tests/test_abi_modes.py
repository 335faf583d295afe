"""The C ABI of the modes is additive: the header still compiles on its own as C99 and as C++ with the new declarations used with
their documented types and the struct laid out as documented, a C host links against them with the library alone, the version stays
5 and slam_pf_config keeps its size; the ctypes table binds both new symbols and the Python layer has its two methods.  Needs no GPU."""
import ctypes as C
import subprocess

from __graft_entry__ import load_package

NEW = ("slam_pf_modes", "slam_pose_modes_dev")

PROGRAM = r'''
#include <stddef.h>
#include "%s"
static int (*const p_modes)(slam_pf *, float, float, int, int, slam_pf_mode *, int *, int *) = slam_pf_modes;
static int (*const p_dev)(slam_engine *, const float *, const float *, const float *, const int32_t *, const float *, int, float,
                          float, int, int, slam_pf_mode *, int *, int *, int64_t *) = slam_pose_modes_dev;
typedef char layout_ok[sizeof(slam_pf_mode) == 40 && offsetof(slam_pf_mode, pose) == 0 && offsetof(slam_pf_mode, mass) == 12 &&
                       offsetof(slam_pf_mode, cell) == 16 && offsetof(slam_pf_mode, ncells) == 28 &&
                       offsetof(slam_pf_mode, weight) == 32 ? 1 : -1];
int main(void)
{
    slam_pf_mode modes[8];
    int n_modes, cells;
    int64_t wtotal;
    layout_ok ok = { 0 };
    (void)ok;
    /* null handles are refused, not dereferenced: no GPU is touched */
    if (p_modes(0, 0.0f, 0.5f, 8, 4, modes, &n_modes, &cells) == SLAM_OK ||
        p_dev(0, 0, 0, 0, 0, 0, 1, 0.0f, 0.5f, 8, 4, modes, &n_modes, &cells, &wtotal) == SLAM_OK)
        return 2;
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


def test_version_bindings_and_layout():
    pkg = load_package()
    lib = pkg.load_library()
    assert lib.slam_abi_version() == 5
    for name in NEW:
        assert name in pkg.SIGNATURES and getattr(lib, name).argtypes == pkg.SIGNATURES[name][1]
    assert len(pkg.SIGNATURES["slam_pf_modes"][1]) == 8 and len(pkg.SIGNATURES["slam_pose_modes_dev"][1]) == 15
    assert callable(pkg.PfSession.modes) and callable(pkg.Engine.pose_modes_dev)
    m = pkg.PfMode
    assert C.sizeof(m) == 40 and (m.pose.offset, m.mass.offset, m.cell.offset, m.ncells.offset, m.weight.offset) == (0, 12, 16, 28, 32)
    text = pkg.HEADER_PATH.read_text()
    assert "#define SLAM_ABI_VERSION 5" in text and all(name + "(" in text for name in NEW) and "} slam_pf_mode;" in text
