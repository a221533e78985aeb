// Test harness (CPU): the integer geometry of batched path IK - ikflow_amd/csrc/path_batch_math.h, the very source the GPU runs - compiled with
// g++ so that tests/test_path_batch_math_host.py can hold it against plain Python without a GPU.  Not part of the product.
#include "../ikflow_amd/csrc/path_batch_math.h"

extern "C" long long pbm_waypoints(long long P, long long T) { return ikf::path_batch_waypoints(P, T); }
extern "C" long long pbm_offset(long long p, long long T) { return ikf::path_batch_offset(p, T); }
extern "C" long long pbm_row(long long P, long long T, long long p, long long t, int r) { return ikf::path_batch_row(P, T, p, t, r); }
extern "C" long long pbm_bp_stride(long long T, int k) { return ikf::path_batch_bp_stride(T, k); }
extern "C" long long pbm_bp_offset(long long p, long long T, int k) { return ikf::path_batch_bp_offset(p, T, k); }
extern "C" long long pbm_bp_bytes(long long P, long long T, int k) { return ikf::path_batch_bp_bytes(P, T, k); }
extern "C" long long pbm_single_bp_bytes(long long T, int k) { return ikf::path_bp_bytes(T, k); }
extern "C" long long pbm_mask_offset(long long p, long long T, int k) { return ikf::path_batch_mask_offset(p, T, k); }
extern "C" long long pbm_pred_row(long long P, long long T, long long g, int j) { return ikf::path_batch_pred_row(P, T, g, j); }
extern "C" long long pbm_word_index(long long g, int r, int word, int k) { return ikf::sweep_word_index(g, r, word, k); }
extern "C" long long pbm_mask_words(long long G, int k) { return ikf::sweep_mask_words(G, k); }
// wave of the sweep's lattice source over a batch -> out = {p, t, r, word}
extern "C" void pbm_wave_role(long long wave, long long T, int k, long long* out) {
  long long g;
  int r, word;
  ikf::sweep_wave_role(wave, k, &g, &r, &word);
  const ikf::PathBatchRole role = ikf::path_batch_role(g, T);
  out[0] = role.p;
  out[1] = role.t;
  out[2] = r;
  out[3] = word;
}
// the words the walk back of a chunk reads from a path's block: (n * k + 3) / 4, as k_path_lattice computes it
extern "C" long long pbm_chunk_words(int n, int k) { return ((long long)n * k + 3) / 4; }
extern "C" int pbm_bt_chunk() { return ikf::IKF_PATH_BT_CHUNK; }
