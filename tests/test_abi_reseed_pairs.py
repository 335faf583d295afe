"""The C ABI of reseeding from detection pairs is additive: the header still compiles on its own as C99 and as C++ with the new
declarations used with their documented types, a C host links against them with the library alone, null handles are refused, the
version stays 5 and slam_pf_config keeps its size; the ctypes table binds the new symbols and the Python layer has its methods; the
single-detection declarations are what they were.  Needs no GPU."""
import ctypes as C
import subprocess

from __graft_entry__ import load_package

NEW = ("slam_pose_reseed_pairs_dev", "slam_pose_reseed_pairs_count", "slam_pf_known_map_reseed_pairs")

PROGRAM = r'''
#include "%s"
static int (*const p_dev)(slam_engine *, const float *, int, int, const float *, const float *, const float *, const int32_t *, float *,
                          float *, float *, int, int64_t, uint64_t, uint32_t, float, float, float, uint8_t *, int32_t[4]) = slam_pose_reseed_pairs_dev;
static int (*const p_count)(slam_engine *, int64_t *) = slam_pose_reseed_pairs_count;
static int (*const p_pf)(slam_pf *, float, float, float, int32_t[4]) = slam_pf_known_map_reseed_pairs;
static int (*const p_single)(slam_pf *, float, int32_t[2]) = slam_pf_known_map_reseed;
int main(void)
{
    int32_t counts[4];
    int64_t launches;
    float v[3] = { 0.0f, 0.0f, 0.0f };
    /* null handles are refused, not dereferenced: no GPU is touched */
    if (p_dev(0, v, 2, 2, v, v, v, 0, v, v, v, 1, 0, 0u, 0u, 0.5f, 0.05f, 1.0f, 0, counts) != SLAM_ERR_INVALID_ARG) return 2;
    if (p_count(0, &launches) != SLAM_ERR_INVALID_ARG || p_pf(0, 0.5f, 0.05f, 1.0f, counts) != SLAM_ERR_INVALID_ARG) return 3;
    if (p_single(0, 0.5f, counts) != SLAM_ERR_INVALID_ARG) return 4;
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
    assert [len(pkg.SIGNATURES[name][1]) for name in NEW] == [20, 2, 5]
    assert [len(pkg.SIGNATURES[name][1]) for name in ("slam_pose_reseed_dev", "slam_pose_reseed_count", "slam_pf_known_map_reseed")] == [18, 2, 3]
    assert callable(pkg.Engine.pose_reseed_pairs_dev) and callable(pkg.Engine.pose_reseed_pairs_count)
    assert callable(pkg.PfSession.known_map_reseed_pairs)
    text = pkg.HEADER_PATH.read_text()
    assert "#define SLAM_ABI_VERSION 5" in text and all(name + "(" in text for name in NEW)
    assert "tests/_reseed_pair_spec.py" in text and "det_atan2" in text
