// Stand-alone host check of the argument handling of csrc/skeleton.hip: every launcher must refuse bad arguments BEFORE it touches
// a buffer or launches, and the pure size functions must take any int.  Built with the host sanitizers it needs no GPU (no call
// below gets as far as the HIP runtime) and no LD_PRELOAD:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -I hyperpri_amd/csrc -x hip hyperpri_amd/csrc/skeleton.hip hyperpri_amd/csrc/api.cpp tools/skeleton_args_check.cpp \
//         -o skeleton_args_check && ./skeleton_args_check
//
// The buffers handed over are small heap blocks with nothing around them: a launcher that read or wrote one on the host, or past
// it, would be reported.  Exit code 0 and "ok" when every call returned what it should.
#include <climits>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/hyperpri_hip.h"

static int failures = 0;

static void expect(bool ok, const char* what) {
  if (!ok) { std::printf("FAIL: %s (last error: %s)\n", what, hpri_last_error()); ++failures; }
}

static void refused(int rc, const char* word, const char* what) {
  expect(rc == -1 && std::strstr(hpri_last_error(), word) != nullptr, what);
}

int main() {
  std::vector<float> f(16, 0.f), g(16, 0.f), o(16, 0.f), sv(5 * 16), ws(4 * 16);
  std::vector<double> st(8), wd(16);
  float loss = 0.f, terms[3] = {0.f, 0.f, 0.f};
  const size_t big = (size_t)1 << 40;

  expect(hpri_soft_skeleton_tile() == 64 && hpri_soft_skeleton_max_iters() == 32, "tile and max_iters");
  expect(hpri_soft_skeleton_lds_bytes(32) == 2u * 132 * 132 * 4 && hpri_soft_skeleton_lds_bytes(-1) == 0 && hpri_soft_skeleton_lds_bytes(INT_MAX) == 0, "lds_bytes");
  expect(hpri_soft_skeleton_saved_floats(1, 4, 4, 2) == 5u * 16 && hpri_soft_skeleton_saved_floats(INT_MAX, 1, 1, 32) == 65 * (size_t)INT_MAX &&
             hpri_soft_skeleton_saved_floats(1, 4, 4, INT_MIN) == 0, "saved_floats");
  expect(hpri_soft_skeleton_workspace_floats(INT_MAX, INT_MAX, 1) == 4 * (size_t)INT_MAX * (size_t)INT_MAX && hpri_soft_skeleton_workspace_floats(INT_MIN, 1, 1) == 0,
         "workspace_floats");
  expect(hpri_cldice_workspace_doubles(1, INT_MAX, INT_MAX) == 4 * ((size_t)1 << 25) * ((size_t)1 << 25) && hpri_cldice_workspace_doubles(1, INT_MIN, 1) == 0,
         "cldice_workspace_doubles");
  expect(hpri_cldice_state_doubles(INT_MAX, 1) == 3 * (size_t)INT_MAX && hpri_cldice_state_doubles(INT_MAX, 0) == 3 && hpri_cldice_state_doubles(0, 1) == 0, "state_doubles");

  refused(hpri_soft_skeleton_fwd(nullptr, 1, 4, 4, 2, o.data(), nullptr, 0, nullptr), "null", "fwd: null p");
  refused(hpri_soft_skeleton_fwd(f.data(), 1, 4, 4, 2, nullptr, nullptr, 0, nullptr), "null", "fwd: null S");
  refused(hpri_soft_skeleton_fwd(f.data(), 0, 4, 4, 2, o.data(), nullptr, 0, nullptr), "sizes", "fwd: N = 0");
  refused(hpri_soft_skeleton_fwd(f.data(), 1, INT_MIN, 4, 2, o.data(), nullptr, 0, nullptr), "sizes", "fwd: h = INT_MIN");
  refused(hpri_soft_skeleton_fwd(f.data(), 1, INT_MAX, 1, 2, o.data(), nullptr, 0, nullptr), "beyond", "fwd: h = INT_MAX");
  refused(hpri_soft_skeleton_fwd(f.data(), INT_MAX, 1, 1, 2, o.data(), nullptr, 0, nullptr), "beyond", "fwd: N = INT_MAX");
  refused(hpri_soft_skeleton_fwd(f.data(), 1, 65536, 65536, 2, o.data(), nullptr, 0, nullptr), "beyond", "fwd: 2^32 pixels");
  refused(hpri_soft_skeleton_fwd(f.data(), 1, 4, 4, -1, o.data(), nullptr, 0, nullptr), "iters", "fwd: iters = -1");
  refused(hpri_soft_skeleton_fwd(f.data(), 1, 4, 4, 33, o.data(), nullptr, 0, nullptr), "iters", "fwd: iters = 33");
  refused(hpri_soft_skeleton_fwd(f.data(), 1, 4, 4, 2, o.data(), sv.data(), sv.size() - 1, nullptr), "saved", "fwd: short saved");

  refused(hpri_soft_skeleton_bwd(f.data(), nullptr, big, g.data(), 1, 4, 4, 2, o.data(), ws.data(), big, nullptr), "null", "bwd: null saved");
  refused(hpri_soft_skeleton_bwd(f.data(), sv.data(), sv.size(), g.data(), 1, 4, 4, 2, o.data(), nullptr, big, nullptr), "null", "bwd: null workspace");
  refused(hpri_soft_skeleton_bwd(f.data(), sv.data(), sv.size(), g.data(), 1, 4, 0, 2, o.data(), ws.data(), ws.size(), nullptr), "sizes", "bwd: w = 0");
  refused(hpri_soft_skeleton_bwd(f.data(), sv.data(), sv.size(), g.data(), 1, 4, 4, 33, o.data(), ws.data(), ws.size(), nullptr), "iters", "bwd: iters = 33");
  refused(hpri_soft_skeleton_bwd(f.data(), sv.data(), sv.size() - 1, g.data(), 1, 4, 4, 2, o.data(), ws.data(), ws.size(), nullptr), "saved", "bwd: short saved");
  refused(hpri_soft_skeleton_bwd(f.data(), sv.data(), sv.size(), g.data(), 1, 4, 4, 2, o.data(), ws.data(), ws.size() - 1, nullptr), "workspace", "bwd: short workspace");

  refused(hpri_cldice_fwd(f.data(), nullptr, 1, 4, 4, 2, 1.f, 0, 1.f, nullptr, 0.f, o.data(), nullptr, g.data(), sv.data(), sv.size(), &loss, terms, st.data(),
                          st.size(), wd.data(), wd.size(), nullptr), "null", "cldice_fwd: null target");
  refused(hpri_cldice_fwd(f.data(), g.data(), 1, 4, 4, 2, -1.f, 0, 1.f, nullptr, 0.f, o.data(), nullptr, g.data(), sv.data(), sv.size(), &loss, terms, st.data(),
                          st.size(), wd.data(), wd.size(), nullptr), "smooth", "cldice_fwd: smooth < 0");
  refused(hpri_cldice_fwd(f.data(), g.data(), 1, 4, 4, 2, 1.f, 1, 1.f, nullptr, 0.f, o.data(), nullptr, g.data(), sv.data(), sv.size(), &loss, terms, st.data(), 2,
                          wd.data(), wd.size(), nullptr), "state", "cldice_fwd: short state");
  refused(hpri_cldice_fwd(f.data(), g.data(), 1, 4, 4, 2, 1.f, 0, 1.f, nullptr, 0.f, o.data(), nullptr, g.data(), sv.data(), sv.size(), &loss, terms, st.data(),
                          st.size(), wd.data(), 3, nullptr), "workspace", "cldice_fwd: short workspace");
  refused(hpri_cldice_fwd(f.data(), g.data(), 1, 4, 4, 40, 1.f, 0, 1.f, nullptr, 0.f, o.data(), nullptr, g.data(), sv.data(), sv.size(), &loss, terms, st.data(),
                          st.size(), wd.data(), wd.size(), nullptr), "iters", "cldice_fwd: iters = 40");

  refused(hpri_cldice_bwd(f.data(), g.data(), f.data(), g.data(), sv.data(), sv.size(), 1, 4, 4, 2, 0, nullptr, 3, nullptr, 0.f, nullptr, o.data(), ws.data(), ws.size(),
                          nullptr), "null", "cldice_bwd: null state");
  refused(hpri_cldice_bwd(f.data(), g.data(), f.data(), g.data(), sv.data(), sv.size(), 1, 4, 4, 2, 1, st.data(), 2, nullptr, 0.f, nullptr, o.data(), ws.data(), ws.size(),
                          nullptr), "state", "cldice_bwd: short state");
  refused(hpri_cldice_bwd(f.data(), g.data(), f.data(), g.data(), sv.data(), sv.size(), 1, 4, 4, 2, 0, st.data(), 3, nullptr, 0.f, nullptr, o.data(), ws.data(),
                          ws.size() - 1, nullptr), "workspace", "cldice_bwd: short workspace");

  std::vector<unsigned char> m(16, 1);
  int counts[4] = {0, 0, 0, 0};
  refused(hpri_centerline_counts(m.data(), m.data(), nullptr, m.data(), 1, 16, counts, nullptr), "null", "centerline_counts: null map");
  refused(hpri_centerline_counts(m.data(), m.data(), m.data(), m.data(), 1, 0, counts, nullptr), "sizes", "centerline_counts: no pixels");
  refused(hpri_centerline_counts(m.data(), m.data(), m.data(), m.data(), INT_MAX, 16, counts, nullptr), "sizes", "centerline_counts: N = INT_MAX");
  refused(hpri_centerline_counts(m.data(), m.data(), m.data(), m.data(), 1, LLONG_MAX, counts, nullptr), "sizes", "centerline_counts: LLONG_MAX pixels");

  if (failures) std::printf("%d check(s) failed\n", failures);
  else std::printf("ok\n");
  return failures ? 1 : 0;
}
