// Stand-alone check of the "once per kernel" bookkeeping (marigold_amd/csrc/kernel_once.h) with a counting setter in place of HIP's:
// 8 threads x 10 000 calls over 4 fake kernel addresses, one of which fails the first time it is set.  Built with
// -fsanitize=thread by tests/test_kernel_once_host.py; exits 0 when every count is right.
#include <stdio.h>

#include <atomic>
#include <map>
#include <thread>
#include <utility>
#include <vector>

#include "../../marigold_amd/csrc/kernel_once.h"

namespace {
constexpr int THREADS = 8, CALLS = 10000, KERNELS = 4, FAILING = 2;
char g_fake_kernels[KERNELS];                        // their addresses are the keys
std::map<std::pair<const void*, int>, int> g_sets;   // (kernel, bytes) -> successful sets; written inside the setter only:
                                                     // the helper's own lock must make that safe
int g_attempts[KERNELS];
std::atomic<int> g_failures{0};

int counting_set(const void* kern, int bytes) {
  const int i = (int)((const char*)kern - g_fake_kernels);
  if (i == FAILING && g_attempts[i]++ == 0) return 1;   // the first attempt on this kernel fails
  if (i != FAILING) g_attempts[i]++;
  g_sets[{kern, bytes}]++;
  return 0;
}

void hammer(mg_kernel_once* once, int bytes, bool dry, int thread) {
  for (int c = 0; c < CALLS; ++c) {
    const void* kern = &g_fake_kernels[(c + thread) % KERNELS];
    if (once->raise(kern, bytes, dry, counting_set)) g_failures++;
  }
}

void run_threads(mg_kernel_once* once, int bytes, bool dry) {
  std::vector<std::thread> ts;
  for (int t = 0; t < THREADS; ++t) ts.emplace_back(hammer, once, bytes, dry, t);
  for (auto& t : ts) t.join();
}

int g_bad = 0;
void expect(bool ok, const char* what) {
  if (!ok) { fprintf(stderr, "kernel_once: FAILED: %s\n", what); g_bad = 1; }
}
int sets(int i, int bytes) { return g_sets[{&g_fake_kernels[i], bytes}]; }
}  // namespace

int main() {
  mg_kernel_once once;
  run_threads(&once, 64 * 1024, true);   // dry run: nothing set, nothing recorded
  expect(g_sets.empty() && g_failures == 0, "the dry run calls no setter");
  run_threads(&once, 64 * 1024, false);
  for (int i = 0; i < KERNELS; ++i) expect(sets(i, 64 * 1024) == 1, "each kernel is set exactly once at the first size");
  expect(g_failures == 1 && g_attempts[FAILING] == 2, "the failed kernel is reported once, retried and then set once");
  for (int i = 0; i < KERNELS; ++i) expect(i == FAILING || g_attempts[i] == 1, "the dry run recorded nothing: one attempt per kernel");
  run_threads(&once, 160 * 1024, false);   // a larger request raises every kernel once more
  run_threads(&once, 64 * 1024, false);    // ... and a smaller one afterwards sets nothing
  for (int i = 0; i < KERNELS; ++i) expect(sets(i, 160 * 1024) == 1 && sets(i, 64 * 1024) == 1, "a larger size raises it once more");
  expect(g_failures == 1 && g_sets.size() == 2 * KERNELS, "no other set, no other failure");
  if (!g_bad) printf("kernel_once: ok\n");
  return g_bad;
}
