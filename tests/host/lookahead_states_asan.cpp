// lookahead_states_asan.cpp -- containment of the look-ahead from caller-supplied state rows, as a stand-alone program for
// AddressSanitizer and UBSan (tests/lookahead_states_host_lib.py build_asan; tests/test_lookahead_states.py runs it as a child process).
// It calls the host entry of lookahead_states_host.cpp on exactly-sized heap buffers with rows that no ss_step state looks like: word 59
// (the target index) 1e9, -5 and NaN, and dynamic words (0..54) NaN and Inf.  No such row may make look_row<Model, true> or obs_from_row
// touch a byte outside the row's own buffers; the non-finite rows are done in their first step.
// usage: lookahead_states_asan FILE KIND   FILE: 64 x 186 f32 states, then 64 x 24 x 21 f32 actions (the case set of lookahead_cases.py)
// TEST INFRASTRUCTURE ONLY, never shipped and never loaded into another process.
#include "lookahead_states_host.cpp"

#include <cmath>
#include <cstdio>
#include <limits>

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  const int kind = std::atoi(argv[2]);
  constexpr int n = 64, H = 24, m = 64;
  std::vector<float> st((size_t)n * SS_STATE_DIM), act((size_t)n * H * SS_ACT_DIM);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  const bool read = std::fread(st.data(), sizeof(float), st.size(), f) == st.size() &&
                    std::fread(act.data(), sizeof(float), act.size(), f) == act.size();
  std::fclose(f);
  if (!read) return 2;

  // row k starts from case k, with the odd rows spoilt
  std::vector<float> rows(st);
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  const float word59[3] = {1e9f, -5.f, nan};
  int nonfinite[m] = {};
  for (int k = 1; k < m; k += 2) {
    float* S = rows.data() + (size_t)k * SS_STATE_DIM;
    const int what = (k / 2) % 5;
    if (what < 3) S[59] = word59[what];
    else {
      for (int i = 0; i < 55; ++i) S[i] = what == 3 ? nan : ((i & 1) ? inf : -inf);
      nonfinite[k] = 1;
    }
  }
  std::vector<int> ids(m);
  for (int k = 0; k < m; ++k) ids[k] = (k * 7) % n;
  ids[5] = n + 2;                                              // a bad id next to the bad rows
  std::vector<float> obs((size_t)m * H * SS_OBS_DIM), rew((size_t)m * H), fs((size_t)m * SS_STATE_DIM), work((size_t)m * SS_LOOK_WORK);
  std::vector<unsigned char> done((size_t)m * H, 0xA5);
  lhs_lookahead_states(kind, n, 21, 3, nullptr, 1.f, st.data(), ids.data(), m, rows.data(), H, act.data(), obs.data(), rew.data(),
                       done.data(), fs.data(), work.data(), nullptr);
  int rc = 0;
  for (int k = 0; k < m; ++k) {
    if (k == 5) {
      if (done[(size_t)k * H] != 0xA5) { std::printf("row %d (bad id) was written\n", k); rc = 1; }
    } else if (nonfinite[k] && done[(size_t)k * H] != 1) {
      std::printf("row %d (non-finite) is not done in its first step\n", k);
      rc = 1;
    }
  }
  std::vector<float> o((size_t)m * SS_OBS_DIM);
  lhs_observe(kind, m, rows.data(), o.data());
  std::printf("%s\n", rc ? "FAILED" : "ok");
  return rc;
}
