// Host test of ikflow_amd/csrc/flow_plan.h: the planner (plan_rows / plan_text) and the cluster form's back-off (ClusterBackoff) without a
// handle or a device, built with plain g++ and -fsanitize=address,undefined (tests/test_flow_plan_host.py).  The plan strings repeat those of
// tests/test_host_logic.py on purpose: that test sees the library, this one the header.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "flow_plan.h"

using namespace ikf;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                             \
    }                                                                      \
  } while (0)

static std::string describe(int n_cu, long long rows, bool ro = true, bool cl = true) {
  return plan_text(plan_rows(rows, n_cu, ro, cl, -1, -1, -1));
}

static void check_strings(const char* got, const char* want) {
  if (std::string(got) != want) {
    fprintf(stderr, "plan: got \"%s\", want \"%s\"\n", got, want);
    exit(1);
  }
}

static void test_decisions_on_256_cus() {
  static const struct { long long rows; const char* want; } table[] = {
      {1, "cluster32:1"}, {8, "cluster32:8"}, {128, "cluster32:128"}, {129, "cluster16:129"}, {256, "cluster16:256"}, {257, "cluster8:257"},
      {512, "cluster8:512"}, {513, "cluster8:512 cluster32:1"}, {600, "cluster8:512 cluster32:88"}, {1024, "cluster4:1024"},
      {1025, "cluster4:1024 cluster32:1"}, {1536, "cluster8:512 cluster4:1024"}, {2048, "cluster2:2048"}, {2049, "cluster2:2048 cluster32:1"},
      {2560, "cluster8:512 cluster2:2048"}, {3072, "cluster4:1024 cluster2:2048"}, {3400, "rowowner:3400"}, {4096, "rowowner:4096"},
      {4097, "rowowner:4096 cluster32:1"}, {4296, "rowowner:4096 cluster16:200"}, {8192, "rowowner:8192"}, {15788, "rowowner:15788"},
      {125000, "rowowner:122880 cluster2:2048 cluster32:72"}};
  static_assert(sizeof(table) / sizeof(table[0]) == 23, "the 23 decisions of test_planner_decisions_and_invariants_host_side");
  for (const auto& t : table) check_strings(describe(256, t.rows).c_str(), t.want);
  check_strings(describe(256, 0).c_str(), "");                                             // 0 rows
  check_strings(describe(256, 300, false, false).c_str(), "perlayer:300");                 // no forms
  check_strings(describe(256, 4096, true, false).c_str(), "rowowner:4096");                // row-owner only
  check_strings(describe(256, 200, true, false).c_str(), "perlayer:200");                  // (a short call: not worth a row-owner round)
  check_strings(describe(256, 4096, false, true).c_str(), "cluster2:2048 cluster2:2048");  // cluster only
  CHECK(plan_rows(10, 0, true, true, -1, -1, -1).empty() && plan_rows(-1, 256, true, true, -1, -1, -1).empty());
}

static bool cluster_form(int f) { return f == 2 || f == 4 || f == 8 || f == 16 || f == 32; }

// what must hold whatever the cost tables say
static void check_invariants(int n_cu, long long rows, const std::vector<FlowChunk>& plan) {
  const long long round = 16LL * n_cu;
  long long sum = 0;
  int rowowner = 0;
  for (size_t i = 0; i < plan.size(); ++i) {
    const FlowChunk& c = plan[i];
    CHECK(c.rows > 0);                                             // no chunk is empty
    sum += c.rows;
    CHECK(c.form == 0 || c.form == 1 || cluster_form(c.form));
    if (c.form >= 2) CHECK((c.rows + 15) / 16 * c.form <= n_cu);   // every cluster grid (row tiles x members) fits the chip
    if (c.form == 1) {
      ++rowowner;
      CHECK(i == 0);                                               // the row-owner chunk comes first
    }
    if (n_cu == 256) CHECK(c.form != 0);                           // the chip the costs were measured on: one weight image for every size
  }
  CHECK(sum == rows);                                              // the chunks add up to the call
  CHECK(rowowner <= 1);
  CHECK(rows < round || (!plan.empty() && plan[0].form == 1));     // a full round always goes to the row-owner launch
}

static void test_invariants_over_three_rounds() {
  for (int n_cu : {8, 64, 240, 256, 304}) {
    const long long round = 16LL * n_cu;
    for (long long rows = 1; rows < 3 * round + 40; ++rows) check_invariants(n_cu, rows, plan_rows(rows, n_cu, true, true, -1, -1, -1));
    check_invariants(n_cu, 10 * round + 5, plan_rows(10 * round + 5, n_cu, true, true, -1, -1, -1));
  }
}

// Without the row-owner launch the cluster form takes the whole batch: full 2-member launches are peeled off iteratively - a million rows
// once overflowed the stack of the recursive tail planner.
static void test_ten_million_rows_cluster_only() {
  const int n_cu = 64;
  const long long rows = 10000000;
  const std::vector<FlowChunk> plan = plan_rows(rows, n_cu, false, true, -1, -1, -1);
  long long sum = 0;
  for (const FlowChunk& c : plan) {
    CHECK(cluster_form(c.form) && c.rows > 0 && (c.rows + 15) / 16 * c.form <= n_cu);
    sum += c.rows;
  }
  CHECK(sum == rows);
}

// ---- the back-off, driven the way plan_flow drives it: a give-up is folded in front of a plan, the plan asks once, then says what it used ----
static bool plan(ClusterBackoff& b, bool wants_cluster = true) {
  const bool may = b.ask();
  b.used(may && wants_cluster);
  return may;
}
// sits out the whole pause (asserting its length), leaving the form allowed again
static void sit_out(ClusterBackoff& b, long long want) {
  CHECK(b.pause_left() == want && b.paused());
  for (long long i = 0; i < want; ++i) {
    CHECK(b.pause_left() == want - i);
    CHECK(!plan(b));
  }
  CHECK(!b.paused() && b.pause_left() == 0);
}

static void test_first_pause() {
  ClusterBackoff b;
  CHECK(!b.paused() && b.pause_left() == 0 && b.repairs() == 0 && plan(b));
  CHECK(!b.give_up(1));
  CHECK(b.repairs() == 1 && b.pause_left() == kClusterFirstPause && kClusterFirstPause == 16);
  // describing a plan (plan_flow without `consume`) only looks: it never consumes the pause
  for (int i = 0; i < 100; ++i) CHECK(b.paused() && b.pause_left() == 16);
  for (int i = 0; i < 16; ++i) CHECK(!b.ask());   // false exactly 16 times,
  CHECK(b.ask());                                 // then true
  CHECK(!b.paused() && b.last_pause() == 16);
}

static void test_doubling_and_cap() {
  ClusterBackoff b;
  long long want = 16;
  for (int n = 1; n <= 20; ++n) {
    CHECK(!b.give_up(1));
    CHECK(b.repairs() == n);
    sit_out(b, want);
    for (int i = 0; i < 5; ++i) CHECK(plan(b));   // fewer than 64 clean cluster plans: the history stays
    want = want * 2 < 65536 ? want * 2 : 65536;
  }
  CHECK(want == 65536 && kClusterMaxPause == 65536 && b.last_pause() == 65536);   // 16 << 12 reached with the 13th give-up, kept since
  CHECK(!b.give_up(1) && b.pause_left() == 65536);
  CHECK(!b.give_up(1) && b.pause_left() == 65536);   // (a give-up folded during a pause starts it over, no longer than the cap)
}

// A plan counts as clean when the NEXT plan asks (the give-up of a launch is only seen in front of the next plan): 64 clean cluster plans are on
// record once the 65th has asked.  If that one's launch gives up, the history is already forgotten.
static void test_clean_streak() {
  CHECK(kClusterCleanStreak == 64);
  for (int clean : {64, 63}) {
    ClusterBackoff b;
    b.give_up(1);
    sit_out(b, 16);
    b.give_up(1);
    sit_out(b, 32);
    for (int i = 0; i < clean; ++i) CHECK(plan(b));   // `clean` cluster plans without a give-up ...
    CHECK(b.clean_streak() == clean - 1);
    CHECK(plan(b));                                   // ... and the plan whose launch gives up
    CHECK(b.clean_streak() == clean);
    b.give_up(1);
    CHECK(b.clean_streak() == 0);
    CHECK(b.pause_left() == (clean == 64 ? 16 : 64));   // 64: forgotten, the first pause again; 63: double the previous
  }
  {
    // the 64th plan's own launch gave up (folded before a 65th asks): 63 clean ones, the pause doubles
    ClusterBackoff b;
    b.give_up(1);
    sit_out(b, 16);
    for (int i = 0; i < 64; ++i) CHECK(plan(b));
    b.give_up(1);
    CHECK(b.pause_left() == 32);
  }
  {
    // plans without a cluster chunk neither count towards the streak nor break it
    ClusterBackoff b;
    b.give_up(1);
    sit_out(b, 16);
    for (int i = 0; i < 40; ++i) CHECK(plan(b, true));
    for (int i = 0; i < 200; ++i) CHECK(plan(b, false));
    CHECK(b.clean_streak() == 40);   // (the 40th cluster plan was counted by the first plan without one)
    for (int i = 0; i < 23; ++i) CHECK(plan(b, true));
    CHECK(plan(b, false));
    CHECK(b.clean_streak() == 63 && b.last_pause() == 16);
    b.give_up(1);
    CHECK(b.pause_left() == 32);
  }
  {
    // nothing on record: nothing is counted
    ClusterBackoff b;
    for (int i = 0; i < 200; ++i) CHECK(plan(b));
    CHECK(b.clean_streak() == 0 && b.last_pause() == 0);
  }
}

// why == 2: a member of the XCD-local form met a peer on another XCD - the caller drops that form, and nothing pauses
static void test_misplaced_local_launch() {
  ClusterBackoff b;
  CHECK(b.give_up(2));
  CHECK(b.repairs() == 1 && !b.paused() && b.pause_left() == 0 && b.last_pause() == 0);
  CHECK(plan(b));
  b.give_up(1);
  sit_out(b, 16);
  for (int i = 0; i < 11; ++i) CHECK(plan(b));
  CHECK(b.clean_streak() == 10);
  CHECK(b.give_up(2));
  CHECK(b.repairs() == 3 && b.clean_streak() == 0 && !b.paused() && b.last_pause() == 16);   // a repair, the streak zeroed, backoff untouched
  CHECK(plan(b));
  CHECK(!b.give_up(1));
  CHECK(b.pause_left() == 32);
}

static void test_forget() {
  ClusterBackoff b;
  b.give_up(1);
  sit_out(b, 16);
  for (int i = 0; i < 8; ++i) CHECK(plan(b));
  b.give_up(1);
  CHECK(b.pause_left() == 32 && b.repairs() == 2);
  b.forget();   // what ikf_load_weights does
  CHECK(!b.paused() && b.pause_left() == 0 && b.last_pause() == 0 && b.clean_streak() == 0);
  CHECK(b.repairs() == 2);   // the give-ups seen so far stay counted
  CHECK(plan(b));
  b.give_up(1);
  CHECK(b.pause_left() == 16 && b.repairs() == 3);
}

int main() {
  test_decisions_on_256_cus();
  test_invariants_over_three_rounds();
  test_ten_million_rows_cluster_only();
  test_first_pause();
  test_doubling_and_cap();
  test_clean_streak();
  test_misplaced_local_launch();
  test_forget();
  printf("flow_plan_host ok\n");
  return 0;
}
