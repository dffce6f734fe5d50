// lookahead_policy_asan.cpp -- the closed-loop look-ahead on the host as a stand-alone program for AddressSanitizer and UBSan
// (tests/lookahead_policy_host_lib.py build_asan; tests/test_lookahead_policy.py runs it as a child process).  It packs a ragged net
// (60 -> 37 -> 50 -> 21: softsign, relu, tanh -- widths that are no multiple of the tile, so that the padding is exercised) into an
// exactly-sized heap buffer and runs the 64 cases of lookahead_cases.py through lhp_lookahead_policy, from the envs and from state rows,
// on exactly-sized output buffers, with one bad id among the rows.
// usage: lookahead_policy_asan FILE KIND   FILE: 64 x 186 f32 states (anything behind them is ignored)
// TEST INFRASTRUCTURE ONLY, never shipped and never loaded into another process.
#include "lookahead_policy_host.cpp"

#include <cstdio>

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  const int kind = std::atoi(argv[2]);
  constexpr int n = 64, H = 24, m = 64;
  std::vector<float> st((size_t)n * SS_STATE_DIM);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  const bool read = std::fread(st.data(), sizeof(float), st.size(), f) == st.size();
  std::fclose(f);
  if (!read) return 2;

  ss_policy_desc d{};
  d.layers = 3;
  const int width[4] = {60, 37, 50, 21};
  const int activation[3] = {SS_POLICY_SOFTSIGN, SS_POLICY_RELU, SS_POLICY_TANH};
  std::vector<std::vector<float>> W(3), B(3);
  const float* wp[3];
  const float* bp[3];
  uint32_t lcg = 12345u;
  auto uni = [&]() { lcg = lcg * 1664525u + 1013904223u; return (float)(lcg >> 8) * (1.f / 8388608.f) - 1.f; };      // [-1, 1)
  for (int l = 0; l < 3; ++l) {
    d.width[l] = width[l];
    d.activation[l] = activation[l];
    W[l].resize((size_t)width[l + 1] * width[l]);
    B[l].resize(width[l + 1]);
    for (float& x : W[l]) x = uni() * 0.3f;
    for (float& x : B[l]) x = uni() * 0.1f;
    wp[l] = W[l].data();
    bp[l] = B[l].data();
  }
  d.width[3] = width[3];
  const long long words = lhp_policy_words(&d);
  if (words <= 0) return 2;
  std::vector<float> packed((size_t)words);
  if (lhp_policy_pack(&d, wp, bp, packed.data())) return 2;

  std::vector<int> ids(m);
  for (int k = 0; k < m; ++k) ids[k] = (k * 7) % n;
  ids[5] = n + 2;                                              // a bad id
  int rc = 0;
  for (int from_rows = 0; from_rows < 2; ++from_rows) {
    std::vector<float> obs((size_t)m * H * SS_OBS_DIM), rew((size_t)m * H), fs((size_t)m * SS_STATE_DIM), work((size_t)m * SS_LOOK_WORK);
    std::vector<float> act((size_t)m * H * SS_ACT_DIM, -7.f), off((size_t)m * H * SS_ACT_DIM);
    for (float& x : off) x = uni() * 0.05f;
    std::vector<unsigned char> done((size_t)m * H, 0xA5);
    lhp_lookahead_policy(kind, n, 21, 3, nullptr, 1.f, st.data(), ids.data(), m, from_rows ? st.data() : nullptr, H, &d, packed.data(),
                         off.data(), act.data(), obs.data(), rew.data(), done.data(), fs.data(), work.data(), nullptr);
    int live = 0;
    for (int k = 0; k < m; ++k) {
      if (k == 5) {
        if (done[(size_t)k * H] != 0xA5 || act[(size_t)k * H * SS_ACT_DIM] != -7.f) { std::printf("row %d (bad id) was written\n", k); rc = 1; }
      } else {
        if (done[(size_t)k * H] > 1) { std::printf("row %d was not written\n", k); rc = 1; }
        live += done[(size_t)k * H + H - 1] == 0;
      }
    }
    std::printf("%s: %d rows live after %d steps\n", from_rows ? "from state rows" : "from the envs", live, H);
  }
  std::printf("%s\n", rc ? "FAILED" : "ok");
  return rc;
}
