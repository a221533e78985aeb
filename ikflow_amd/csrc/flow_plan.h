// Host arithmetic in front of every flow call: which of the three kernel forms runs which rows (plan_rows), and when a handle may use the
// cluster form again after one of its launches gave up (ClusterBackoff).  No HIP header, no handle, no device: api_flow.hip applies it to a
// handle, tests/flow_plan_host.cpp runs it under the sanitizers without a GPU.
#pragma once
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

namespace ikf {

constexpr int IKF_RO_ROWS = 16;  // rows per workgroup of the resident-row forms (row-owner, cluster)

// ---- which form runs which rows of a batch -------------------------------------------------------------------------------------------
// Three forms compute the same function: the per-layer kernels (any shape), the row-owner launch (a round of CUs x 16 rows costs the same
// whatever part of it is used) and the cluster form (G = 8 / 4 / 2: <= 512 / 1024 / 2048 rows at a fixed cost each).  A batch is cut into
// consecutive chunks by the cheapest plan under the measured costs of the released 12-block shape on 256 CUs (ms per launch,
// tools/rowowner_ab.py, profiles/r04_rowowner_ab.jsonl) - the ratios, not the absolute values, decide, and they hold for any depth:
//   row-owner round 2.82;  cluster 0.285 / 0.335 / 0.485 / 0.82 / 1.51 for G = 32 / 16 / 8 / 4 / 2 (<= 128 / 256 / 512 / 1024 / 2048 rows; r05);
//   per-layer 0.272 / 0.305 / 0.316 / 0.367 / 0.52 / 0.71 / 1.04 / 1.75 / 2.56 / 2.62 / 3.20 up to 1 / 16 / 64 / 128 / 256 / 512 / 1024 /
//   2048 / 2560 / 3072 / 4096 rows (+ 0.10 beside the resident-row forms: another weight image, see plan_tail);  + 0.01 per extra chunk.
// e.g. 1 .. 128 -> cluster 32; 200 -> cluster 16; 512 -> cluster 8; 600 -> cluster 4; 1536 -> cluster 4 (1024) + cluster 8 (512); 2304 -> cluster 2 (2048) + per-layer (256);
// 3400 -> one row-owner round; 4096 k + r -> k rounds in one row-owner launch + the plan of r.
struct FlowChunk {
  int form;         // 0 per-layer, 1 row-owner, 2 / 4 / 8 / 16 / 32 cluster members
  long long rows;
};
// The measured costs, ms per launch (the comment above says where they come from).
struct PerLayerCost { long long rows; double ms; };   // up to `rows` rows of a 256-CU chip
struct ClusterCost { int G; double ms; };
constexpr double kRowOwnerRoundMs = 2.82;
constexpr ClusterCost kClusterMs[] = {{32, 0.285}, {16, 0.335}, {8, 0.485}, {4, 0.82}, {2, 1.51}};   // (r05: tagged hand-over for G <= 16)
constexpr PerLayerCost kPerLayerMs[] = {{1, 0.272}, {16, 0.305}, {64, 0.316}, {128, 0.367}, {256, 0.52}, {512, 0.71}, {1024, 1.04},
                                        {2048, 1.75}, {2560, 2.56}, {3072, 2.62}, {4096, 3.20}};
constexpr double kOtherImageMs = 0.10;   // per-layer kernels beside a resident-row form: the cache holds the other weight image (plan_tail)
constexpr double kExtraChunkMs = 0.01;   // every chunk after the first

inline double per_layer_cost(long long rows_on_256) {
  for (const PerLayerCost& e : kPerLayerMs)
    if (rows_on_256 <= e.rows) return e.ms;
  constexpr PerLayerCost last = kPerLayerMs[sizeof(kPerLayerMs) / sizeof(kPerLayerMs[0]) - 1];   // beyond the table: in proportion
  return last.ms * (double)rows_on_256 / (double)last.rows;
}
// cheapest plan for `rows` rows below one row-owner round; returns its cost, appends its chunks.  Only the forms of G <= 8 (>= 512 rows
// per launch) are taken as a full launch in front of a rest - the small forms only for a whole (rest of a) tail - and results are memoised
// by the remaining row count: a handful of states, a few microseconds per call (an unbounded search over 128-row pieces is exponential).
struct TailPlan {
  double cost;
  std::vector<FlowChunk> chunks;
};
// The per-layer kernels read their own weight images (2 x 203 MB beside the row-owner stream's 203 MB; the Infinity Cache holds 256 MB): next
// to a chunk of another form (mixed), or on a handle whose other calls use the cluster form (cl), they find the cache holding the other
// image and leave it holding theirs - measured + 0.07 ... 0.1 ms on a 513- / 1025- / 2049-row call whose last row went to them.  They are
// charged for it, so that where the resident-row forms are allowed EVERY size reads one image (1 row alone: 0.273 against cluster32's 0.277;
// an exact-IK call on one pose runs rounds of 1, 3, 10 rows); they remain what a handle without those forms, or another shape, runs.
inline const TailPlan& plan_tail(long long rows, long long round, bool ro, bool cl, bool mixed, std::unordered_map<long long, TailPlan>& memo) {
  auto it = memo.find(rows);
  if (it != memo.end()) return it->second;
  TailPlan best{0.0, {}};
  if (rows > 0) {
    const long long on256 = rows * 4096 / round;   // the cost tables are in rows of a 256-CU chip
    best = TailPlan{per_layer_cost(on256) + ((mixed || cl) ? kOtherImageMs : 0.0), {{0, rows}}};
    if (ro && kRowOwnerRoundMs < best.cost) best = TailPlan{kRowOwnerRoundMs, {{1, rows}}};
    if (cl) {
      for (const ClusterCost& f : kClusterMs) {
        const long long cap = (round / IKF_RO_ROWS) / f.G * IKF_RO_ROWS;   // rows of a full grid of this form: whole tiles, at most one workgroup per CU
        if (cap <= 0) continue;
        if (rows <= cap) {                   // the whole tail in one launch of this form
          if (f.ms < best.cost) best = TailPlan{f.ms, {{f.G, rows}}};
        } else if (f.G <= 8) {               // a full launch of this form, then the plan of what is left
          const TailPlan rest = plan_tail(rows - cap, round, ro, cl, true, memo);   // (by value: the map may rehash)
          const double c = f.ms + kExtraChunkMs + rest.cost;
          if (c < best.cost) {
            best = TailPlan{c, {{f.G, cap}}};
            best.chunks.insert(best.chunks.end(), rest.chunks.begin(), rest.chunks.end());
          }
        }
      }
    }
  }
  return memo.emplace(rows, std::move(best)).first->second;
}
// ro / cl: the form may be used at all; ro_mode / cl_mode 1: forced; ro_min_tail >= 0: the probes' explicit threshold for the last partial round
inline std::vector<FlowChunk> plan_rows(long long rows, int n_cu, bool ro, bool cl, int ro_mode, int cl_mode, long long ro_min_tail) {
  std::vector<FlowChunk> plan;
  if (rows <= 0 || n_cu <= 0) return plan;
  const long long round = (long long)n_cu * IKF_RO_ROWS;
  if (ro && ro_mode == 1) return {{1, rows}};
  if (cl && cl_mode == 1 && rows <= round / 2) {  // forced: one launch of the widest form whose grid fits
    for (int g = 32; g >= 2; g /= 2)
      if (rows <= (long long)(n_cu / g) * IKF_RO_ROWS) return {{g, rows}};
  }
  long long full = ro ? rows / round * round : 0;
  if (!ro && cl && rows > round) {
    // no row-owner launch to take the full rounds: whole 2-member cluster launches (the cheapest form per row) are peeled off here, one
    // chunk each, and plan_tail only sees what is left below a round (its recursion is one level per full launch)
    const long long cap2 = (round / IKF_RO_ROWS) / 2 * IKF_RO_ROWS;
    while (cap2 > 0 && rows - full > round) {
      plan.push_back({2, cap2});
      full += cap2;
    }
  }
  const bool peeled = !ro && full > 0;
  std::vector<FlowChunk> tail;
  if (rows - full > 0) {
    if (ro && ro_min_tail >= 0) {
      if (rows - full >= ro_min_tail) tail = {{1, rows - full}};
      else tail = {{0, rows - full}};
    } else {
      std::unordered_map<long long, TailPlan> memo;
      tail = plan_tail(rows - full, round, ro, cl, full > 0, memo).chunks;
    }
  }
  if (full > 0 && !peeled) plan.push_back({1, full});
  for (const FlowChunk& c : tail) {
    if (!plan.empty() && plan.back().form == 1 && c.form == 1) plan.back().rows += c.rows;   // the partial round rides in the same launch
    else plan.push_back(c);
  }
  return plan;
}
// "rowowner:4096 cluster16:200"
inline std::string plan_text(const std::vector<FlowChunk>& plan) {
  std::string out;
  for (const FlowChunk& c : plan) {
    if (!out.empty()) out += " ";
    out += (c.form == 0 ? std::string("perlayer") : c.form == 1 ? std::string("rowowner") : "cluster" + std::to_string(c.form)) + ":" + std::to_string(c.rows);
  }
  return out;
}

// ---- the cluster form's back-off ----------------------------------------------------------------------------------------------------
// A wait of a cluster launch that ran out means a peer was not resident - another process's kernel held CUs just then.  That tenant may be
// gone a second later, so the form is not switched off for good: it sits out kClusterFirstPause plans (ikf_generate_* calls) after the first
// give-up and twice as many after every further one (at most kClusterMaxPause); kClusterCleanStreak plans with the form in a row without a
// give-up forget the history.  A member of the XCD-local form that met a peer on another XCD (why == 2) is no such event: the caller goes
// back to the spread form and nothing pauses.
constexpr long long kClusterFirstPause = 16, kClusterMaxPause = 65536;
constexpr int kClusterCleanStreak = 64;
struct ClusterBackoff {
  // A launch gave up (why: the word it left, 1 a wait ran out, 2 misplaced XCD-local launch).  True: the caller drops the XCD-local form.
  bool give_up(int why) {
    ++repairs_;
    clean_ = 0;
    if (why == 2) return true;
    backoff_ = backoff_ == 0 ? kClusterFirstPause : (backoff_ * 2 < kClusterMaxPause ? backoff_ * 2 : kClusterMaxPause);   // sit out, twice as long as the last time
    pause_ = backoff_;
    return false;
  }
  // Asked once per plan that is about to run: counts the previous plan towards the clean streak and the pause down.  True: the form may be used.
  bool ask() {
    if (used_last_ && pause_ == 0 && backoff_ != 0 && ++clean_ >= kClusterCleanStreak) backoff_ = 0;
    used_last_ = false;
    if (pause_ > 0) {
      --pause_;
      return false;
    }
    return true;
  }
  void used(bool cluster_chunk) { used_last_ = cluster_chunk; }   // the plan that ask() was called for contains a cluster chunk
  bool paused() const { return pause_ > 0; }                      // (what a plan that is only described goes by: consumes nothing)
  long long pause_left() const { return pause_; }
  long long repairs() const { return repairs_; }
  // new weights: no pause, no history; the give-ups seen so far stay counted
  void forget() {
    pause_ = backoff_ = 0;
    clean_ = 0;
  }
  long long last_pause() const { return backoff_; }
  int clean_streak() const { return clean_; }

 private:
  long long pause_ = 0;      // plans the form still sits out
  long long backoff_ = 0;    // length of the last pause (0: no give-up on record)
  int clean_ = 0;            // cluster plans since the last give-up
  bool used_last_ = false;   // the previous plan contained a cluster launch
  long long repairs_ = 0;    // give-ups seen so far (ikf_cluster_repairs)
};

}  // namespace ikf
