// The model-image loader's host code under a sanitizer, without Python and without a GPU: every file on the command line is loaded in
// the host-only mode (mg_model_load(path, -1): parsed, checked and relocated against fake addresses), a file that loads is taken
// through every query, selection and replication the library has, and each outcome is printed.  Good and corrupt files alike must
// end in a line of this program, never in a crash or a sanitizer report (tests/test_model_configs_host.py::corrupt_images makes the
// corrupt ones).  Build the library's sources and this file with the sanitizer on the host side only, and run it on the CPU:
//     make -C marigold_amd/csrc HIPCC="hipcc -Xarch_host -fsanitize=address,undefined -g" BUILD=build_asan \
//          OUT=../libmarigold_hip_asan.so ../libmarigold_hip_asan.so
//     hipcc -O1 -g -std=c++17 -fsanitize=address,undefined -Iinclude tools/model_image_check.cpp -Lmarigold_amd -lmarigold_hip_asan \
//           -Wl,-rpath,$PWD/marigold_amd -o model_image_check
//     ./model_image_check good.mgimg corrupt0.mgimg corrupt1.mgimg ...
// Exit status: 0 when every file either loaded and passed every step or was refused with an "mg_model_load:" message (a file that
// loads and then fails a step, such as a corrupt op that mg_model_validate names, counts as a failure of the file, not of the loader).
#include <stdio.h>
#include <string.h>

#include "marigold_hip.h"

// The steps on a loaded image; -> the step that failed, or null.  The handles it makes are the caller's to destroy.
static const char* steps(mg_model* m, mg_model** r, mg_model** rr, int* n_out, long long* shared, long long* priv) {
  const int n = *n_out = mg_model_num_configs(m);
  int cfg[MG_CFG_WORDS], sel[MG_CFG_WORDS];
  if (n < 1) return "mg_model_num_configs";
  for (int i = 0; i < n; ++i) {
    if (mg_model_config_info(m, i, cfg)) return "mg_model_config_info";
    if (mg_model_select(m, i) || mg_model_info(m, sel) || memcmp(cfg, sel, sizeof(cfg))) return "mg_model_select / mg_model_info";
    if (mg_model_validate(m)) return "mg_model_validate";
    const int found = mg_model_find_config(m, cfg[MG_CFG_HEIGHT], cfg[MG_CFG_WIDTH], cfg[MG_CFG_MEMBERS], cfg[MG_CFG_STEPS], MG_CFG_PICTURES_OF(cfg));
    if (found < 0 || found > i) return "mg_model_find_config";
  }
  if (mg_model_config_info(m, n, cfg) == 0 || mg_model_select(m, n) == 0 || mg_model_select(m, -1) == 0) return "an index out of range was taken";
  if (mg_model_find_config(m, 1, 1, -1, -1, -1) != -1) return "mg_model_find_config (no match)";
  int H = 0, W = 0;
  if (mg_processed_size(375, 1242, 768, &H, &W) || H != 231 || W != 768) return "mg_processed_size";
  // replicas: made, queried, replicated again, validated on every configuration
  *shared = mg_model_shared_bytes(m);
  *priv = mg_model_device_bytes(m);
  if (!(*r = mg_model_replica(m))) return "mg_model_replica";
  if (mg_model_shared_bytes(*r) != *shared || mg_model_device_bytes(*r) != *priv || mg_model_num_configs(*r) != n) return "the replica's accounting";
  if (!(*rr = mg_model_replica(*r))) return "mg_model_replica (of a replica)";
  for (int i = 0; i < n; ++i)
    if (mg_model_select(*rr, i) || mg_model_validate(*rr) || mg_model_select(*r, n - 1 - i) || mg_model_validate(*r)) return "a replica's validation";
  return nullptr;
}

static int check(const char* path) {
  mg_model* m = mg_model_load(path, -1);
  if (!m) {
    const bool named = strncmp(mg_last_error(), "mg_model_load:", 14) == 0;
    printf("%s: refused - %s\n", path, mg_last_error());
    return named ? 0 : 1;
  }
  mg_model *r = nullptr, *rr = nullptr;
  int n = 0;
  long long shared = 0, priv = 0;
  const char* failed = steps(m, &r, &rr, &n, &shared, &priv);
  if (failed) printf("%s: FAILED at %s: %s\n", path, failed, mg_last_error());
  mg_model_destroy(m);   // the parent first: the replicas go on
  if (!failed && (mg_model_shared_bytes(r) != shared || mg_model_num_configs(rr) != n || mg_model_validate(r) || mg_model_validate(rr))) {
    printf("%s: FAILED after the parent was destroyed: %s\n", path, mg_last_error());
    failed = "";
  }
  mg_model_destroy(rr);
  mg_model_destroy(r);
  if (!failed)
    printf("%s: %d configuration(s), %lld shared + %lld private bytes, every query, selection and replica passed\n", path, n, shared, priv);
  return failed ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s image.mgimg [more.mgimg ...]\n", argv[0]);
    return 2;
  }
  int bad = 0;
  for (int i = 1; i < argc; ++i) bad += check(argv[i]);
  if (mg_model_replica(nullptr) || mg_model_num_configs(nullptr) != 0 || mg_model_shared_bytes(nullptr) != 0) bad += 1;
  printf("%d file(s), %d failure(s)\n", argc - 1, bad);
  return bad ? 1 : 0;
}
