"""The C ABI of the localise stage's misses is additive: the header still compiles on its own as C99 and as C++ with the new
declarations used with their documented types, a C host links against them with the library alone, the version stays 5 and
slam_pf_config keeps its size; null handles and null arguments are refused, not dereferenced; the ctypes table binds every new
symbol.  Needs no GPU."""
import ctypes as C
import subprocess

from __graft_entry__ import load_package

NEW = ("slam_localise_miss_dev", "slam_localise_detcov_miss_dev", "slam_localise_miss_count", "slam_pf_known_map_miss_set",
       "slam_pf_known_map_miss_device_view")

PROGRAM = r'''
#include "%s"
typedef int (*stage_fn)(slam_engine *, const float *, int, int, const float *, const float *, const float *, int, float, uint8_t *,
                        int, int32_t *, float *, const slam_localise_view *, int32_t *, int32_t *, int32_t *);
static const stage_fn p_stage = slam_localise_miss_dev;
static const stage_fn p_detcov = slam_localise_detcov_miss_dev;
static int (*const p_count)(slam_engine *, int64_t *) = slam_localise_miss_count;
static int (*const p_set)(slam_pf *, float, float, int, float, float, float, int, float) = slam_pf_known_map_miss_set;
static int (*const p_view)(slam_pf *, const int32_t **, const int32_t **, const int32_t **) = slam_pf_known_map_miss_device_view;
int main(void)
{
    int64_t count;
    int32_t missed[1];
    const slam_localise_view view = { 5.0f, 0.0f, 4.0f, 0, 0.0f };
    /* null handles are refused, not dereferenced: no GPU is touched */
    if (p_count(0, &count) == SLAM_OK || p_set(0, -1.0f, 5.0f, 0, 0.0f, 0.0f, 0.0f, 0, 0.0f) == SLAM_OK || p_view(0, 0, 0, 0) == SLAM_OK) return 2;
    if (p_stage(0, 0, 0, 0, 0, 0, 0, 0, 1.0f, 0, 0, 0, 0, &view, missed, 0, 0) == SLAM_OK) return 3;
    if (p_detcov(0, 0, 0, 0, 0, 0, 0, 0, 1.0f, 0, 0, 0, 0, &view, missed, 0, 0) == SLAM_OK) return 4;
    return slam_abi_version() == SLAM_ABI_VERSION && SLAM_ABI_VERSION == 5 && sizeof(slam_pf_config) == %d &&
           sizeof(slam_localise_view) == 5 * sizeof(float) ? 0 : 1;
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
    assert len(pkg.SIGNATURES["slam_localise_miss_dev"][1]) == len(pkg.SIGNATURES["slam_localise_dev"][1]) + 4
    assert C.sizeof(pkg.LocaliseView) == 20 and [f[0] for f in pkg.LocaliseView._fields_] == ["view_range", "lo", "hi", "sight", "margin"]
    text = pkg.HEADER_PATH.read_text()
    assert "#define SLAM_ABI_VERSION 5" in text and all(name + "(" in text for name in NEW) and "slam_localise_view;" in text
    assert "miss terms" not in " ".join(text.replace("*", " ").split())   # no longer out of scope anywhere in the header
