// Host-only home of the conv dispatch state: the per-family path modes
// (vsrk_conv_set_path / vsrk_conv_get_path), the grid cap and rolling depth
// test knobs, the cached CU count and the environment helpers.  Everything
// here is resolved once, when the library is loaded; the launch paths read
// plain ints (vsrk_path_mode, vsrk_internal.h).  This is the only file of
// csrc that reads the environment or asks the device for its CU count.
#include <cstdlib>
#include <cstring>
#include <string>
#include "vsrk_internal.h"

int vsrk_env_flag(const char* name, int dflt) {
  const char* e = getenv(name);
  return !e ? dflt : (e[0] == '0' ? 0 : 1);
}

int vsrk_env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}

int vsrk_num_cus() {
  static const int n = [] {
    int dev = 0, cus = 0;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    return cus;
  }();
  return n;
}

int vsrk_g_path_mode[VSRK_PATH_COUNT];  // filled below, at load
// The wide row conv's switch (conv_row_wide.hip) is a knob of its own, read
// from VSRK_CONV_ROW_WIDE by the table's rule: the table of named paths is
// pinned by tests/test_paths_cpu.py.  -1: the shapes that measured faster
// than the tile kernel, 0 off, 1 every eligible shape.
int vsrk_g_row_wide_mode;

namespace {

struct PathInfo {
  const char* name;
  const char* env;
  int unset;    // mode when the variable is not set
  int max_set;  // largest mode vsrk_conv_set_path accepts
};

// indexed by vsrk_path
constexpr PathInfo kPaths[VSRK_PATH_COUNT] = {
    {"fast", "VSRK_CONV_FAST", 1, 1},
    {"pw", "VSRK_CONV_PW", 1, 1},
    {"pw_wide", "VSRK_PW_WIDE", 1, 1},
    {"roll", "VSRK_CONV_ROLL", 2, 1},      // 2: automatic (skips shallow output depths), 1: every eligible shape
    {"roll_wr", "VSRK_ROLL_WRES", 1, 2},   // 2: also with the prefetched residual / mask epilogue (tests)
    {"roll_fold", "VSRK_ROLL_FOLD", 1, 1},
    {"row", "VSRK_CONV_ROW", -1, 1},       // -1: the forms that measured faster than the tile kernel
    {"thin", "VSRK_CONV_THIN", 1, 1},
    {"stencil", "VSRK_CONV_STENCIL", 1, 1},
    {"wgrad_pipe", "VSRK_WGRAD_PIPE", 1, 1},
    {"wgrad_roll", "VSRK_WGRAD_ROLL", 2, 1},  // as roll
    {"wgrad_row", "VSRK_WGRAD_ROW", 1, 2},    // 2: also the sub-pixel tap skip forms
};

int g_load_mode[VSRK_PATH_COUNT];  // the modes resolved at load (what mode -1 restores)
int g_row_wide_load;               // ... and of vsrk_conv_set_row_wide

const bool g_paths_loaded = [] {
  for (int i = 0; i < VSRK_PATH_COUNT; ++i)
    vsrk_g_path_mode[i] = g_load_mode[i] = vsrk_env_flag(kPaths[i].env, kPaths[i].unset);
  vsrk_g_row_wide_mode = g_row_wide_load = vsrk_env_flag("VSRK_CONV_ROW_WIDE", -1);
  return true;
}();

int find_path(const char* path) {
  for (int i = 0; i < VSRK_PATH_COUNT; ++i)
    if (strcmp(path, kPaths[i].name) == 0) return i;
  std::string names;
  for (const PathInfo& p : kPaths) names += (names.empty() ? "" : ", ") + std::string(p.name);
  vsrk_set_error("conv path: unknown path '%s' (%s)", path, names.c_str());
  return -1;
}

}  // namespace

int vsrk_g_grid_cap = 0;  // vsrk_conv_set_grid_cap: 0 = one workgroup per CU
int vsrk_g_roll_dz = 0;   // vsrk_conv_set_roll_depth: > 0 output depths per tile of both rolling kernels, 0 automatic
const int vsrk_g_roll_prio = vsrk_env_int("VSRK_ROLL_PRIO", 0) == 1;

extern "C" int vsrk_conv_set_path(const char* path, int32_t mode) {
  VSRK_CHECK(path, "conv_set_path: null path");
  const int i = find_path(path);
  if (i < 0) return VSRK_ERR_INVALID;
  VSRK_CHECK(mode >= -1 && mode <= kPaths[i].max_set, "conv_set_path: %s mode %d outside [-1, %d]", path, mode,
             kPaths[i].max_set);
  vsrk_g_path_mode[i] = mode < 0 ? g_load_mode[i] : mode;
  return VSRK_OK;
}

extern "C" int vsrk_conv_get_path(const char* path, int32_t* mode) {
  VSRK_CHECK(path && mode, "conv_get_path: null argument");
  const int i = find_path(path);
  if (i < 0) return VSRK_ERR_INVALID;
  *mode = vsrk_g_path_mode[i];
  return VSRK_OK;
}

extern "C" int vsrk_conv_set_row_wide(int32_t mode) {
  VSRK_CHECK(mode >= -1 && mode <= 1, "conv_set_row_wide: mode %d outside [-1, 1]", mode);
  vsrk_g_row_wide_mode = mode < 0 ? g_row_wide_load : mode;
  return VSRK_OK;
}

extern "C" int vsrk_conv_get_row_wide(int32_t* mode) {
  VSRK_CHECK(mode, "conv_get_row_wide: null argument");
  *mode = vsrk_g_row_wide_mode;
  return VSRK_OK;
}

extern "C" int vsrk_conv_set_algo(int32_t mode) { return vsrk_conv_set_path("fast", mode); }

extern "C" int vsrk_conv_set_grid_cap(int32_t max_workgroups) {
  VSRK_CHECK(max_workgroups >= 0, "conv_set_grid_cap: max_workgroups must be >= 0");
  vsrk_g_grid_cap = max_workgroups;
  return VSRK_OK;
}

extern "C" int vsrk_conv_set_roll_depth(int32_t depths) {
  VSRK_CHECK(depths >= 0, "conv_set_roll_depth: depths must be >= 0");
  vsrk_g_roll_dz = depths;
  return VSRK_OK;
}
