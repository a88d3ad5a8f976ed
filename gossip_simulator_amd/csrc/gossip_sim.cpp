// gossip_sim -- drop-in for `go run simulator.go` on an MI355X.
//
// Same seven flags, defaults and stdout lines as simulator.go:186-253, driven
// through the C ABI (include/gossip.h).  Durations are SIMULATED time
// (1 tick = 1 ms, the unit of simulator.go:167) printed with Go's
// time.Duration format; wall-clock figures go to stderr.  Additive flags
// (-seed -trial -trials -device -peers -maxticks -model -k -batch -packed -rumors -payload -pick -every) are not
// echoed in
// the parameter block, so stdout keeps the reference's shape.  -model pushpull
// -rumors R runs R rumors from keyed senders as one rumor set
// (gs_create_rumorset): each poll's line shows the least-covered started rumor,
// then one line per rumor and the round at which all were covered; with
// -payload B, -pick low|high|rotate or -every E the set is a bounded one
// (DESIGN.md section 4.9.1): a message carries at most B rumors, rumor j enters
// at round j * E, every rumor's line adds its start and its rounds from there to
// 99 %, and a last line gives the rumor copies wanted and carried.  -model rumor
// and -model median run to their own end and add the residue and the messages
// per node (-model median: one trial, or -batch T trials through
// gs_create_batch, printed like the rumor model's with a stranded column: the
// nodes still active at the trial's stop; -packed sets GS_FLAG_MEDIAN_PACKED for
// the batch, which lets n reach the default 50,000).  -trials T > 1 runs
// T independent trials in one batched context and prints one line per trial;
// with -model rumor (gs_create_trials) the trial lines carry the model's own
// figures and a summary line their mean and sample standard deviation, and
// the exit status is 0 if every trial ended by itself (covered or quiescent),
// 3 if one reached -maxticks.
#include <chrono>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "gossip.h"

namespace {

struct Flag {
  const char* name;
  const char* type;  // Go UnquoteUsage type name
  const char* usage;
  std::string defv;  // Go default as printed
  bool echo;         // part of the reference's flag set (echoed, :197-204)
  std::string val;
  bool given = false;  // set on the command line
};

std::vector<Flag> g_flags;
const char* g_prog = "gossip_sim";

Flag* find(const std::string& name) {
  for (auto& f : g_flags)
    if (name == f.name) return &f;
  return nullptr;
}

std::string gofloat(double x) {
  char b[64];
  gs_format_float64(x, b, sizeof(b));
  return b;
}

void usage() {  // flag.PrintDefaults, lexical order
  fprintf(stderr, "Usage of %s:\n", g_prog);
  std::map<std::string, Flag*> sorted;
  for (auto& f : g_flags) sorted[f.name] = &f;
  for (auto& kv : sorted) {
    Flag* f = kv.second;
    std::string b = std::string("  -") + f->name;
    if (f->type[0] && strcmp(f->type, "bool")) b += std::string(" ") + f->type;  // Go names no type for a bool
    b += (b.size() <= 4) ? "\t" : "\n    \t";
    b += f->usage;
    const bool zero = f->defv == "0" || f->defv.empty() || f->defv == "false";
    if (!zero) {
      if (!strcmp(f->type, "string")) b += " (default \"" + f->defv + "\")";
      else b += " (default " + f->defv + ")";
    }
    fprintf(stderr, "%s\n", b.c_str());
  }
}

[[noreturn]] void die_usage(const std::string& msg) {
  fprintf(stderr, "%s\n", msg.c_str());
  usage();
  exit(2);
}

bool parse_int(const std::string& s, long long& out) {  // strconv.ParseInt(s, 0, 64)
  std::string t;
  for (char ch : s) if (ch != '_') t.push_back(ch);
  if (t.empty()) return false;
  char* end = nullptr;
  errno = 0;
  out = strtoll(t.c_str(), &end, 0);
  return errno == 0 && end && *end == 0;
}

bool parse_float(const std::string& s, double& out) {
  if (s.empty()) return false;
  char* end = nullptr;
  out = strtod(s.c_str(), &end);
  return end && *end == 0;
}

// Go flag.Parse semantics (ExitOnError): -name=v, -name v, --name; stops at
// the first non-flag or after "--"; -h/-help prints usage and exits 0.
void parse(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i];
    if (a.size() < 2 || a[0] != '-') break;
    if (a == "--") break;
    std::string body = a.substr(a[1] == '-' ? 2 : 1);
    if (body.empty() || body[0] == '-' || body[0] == '=')
      die_usage("bad flag syntax: " + a);
    std::string name = body, value;
    bool has = false;
    const size_t eq = body.find('=');
    if (eq != std::string::npos) { name = body.substr(0, eq); value = body.substr(eq + 1); has = true; }
    Flag* f = find(name);
    if (!f) {
      if (name == "h" || name == "help") { usage(); exit(0); }
      die_usage("flag provided but not defined: -" + name);
    }
    f->given = true;
    if (!has && !strcmp(f->type, "bool")) {  // -name alone sets a bool; -name=false clears it
      value = "true";
      has = true;
    }
    if (!has) {
      if (i + 1 >= argc) die_usage("flag needs an argument: -" + name);
      value = argv[++i];
    }
    if (!strcmp(f->type, "int") || !strcmp(f->type, "uint")) {
      long long v;
      if (!parse_int(value, v) || (!strcmp(f->type, "uint") && v < 0))
        die_usage("invalid value \"" + value + "\" for flag -" + name + ": parse error");
      f->val = std::to_string(v);
    } else if (!strcmp(f->type, "float")) {
      double v;
      if (!parse_float(value, v))
        die_usage("invalid value \"" + value + "\" for flag -" + name + ": parse error");
      f->val = gofloat(v);
    } else if (!strcmp(f->type, "bool")) {
      if (value != "true" && value != "false" && value != "1" && value != "0")
        die_usage("invalid boolean value \"" + value + "\" for -" + name + ": parse error");
      f->val = value == "true" || value == "1" ? "true" : "false";
    } else {
      f->val = value;
    }
  }
}

long long ival(const char* n) { return strtoll(find(n)->val.c_str(), nullptr, 10); }
double fval(const char* n) { return strtod(find(n)->val.c_str(), nullptr); }

std::string dur_ms(uint64_t ticks) {
  char b[64];
  gs_format_duration((int64_t)ticks * 1000000ll, b, sizeof(b));
  return b;
}

int die(gs_ctx* c, int rc, const char* what) {
  fprintf(stderr, "%s: %s failed: %s (%s)\n", g_prog, what, gs_strerror(rc),
          c ? gs_last_error(c) : "");
  if (c) gs_destroy(c);
  return 1;
}

// Injected peer table (DESIGN.md "peer-table file"): "GSPEERS1", u64 n,
// u32 stride, u32 reserved, u8 deg[n], pad to 4, u32 ids[n*stride].
bool load_peers_file(const std::string& path, uint64_t n, std::vector<uint8_t>& deg,
                     std::vector<uint32_t>& ids, uint32_t& stride) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) { fprintf(stderr, "%s: cannot open %s\n", g_prog, path.c_str()); return false; }
  char magic[8];
  uint64_t fn = 0;
  uint32_t hdr[2] = {0, 0};
  bool ok = fread(magic, 1, 8, f) == 8 && !memcmp(magic, "GSPEERS1", 8) &&
            fread(&fn, 8, 1, f) == 1 && fread(hdr, 4, 2, f) == 2;
  if (ok && fn != n) {
    fprintf(stderr, "%s: %s holds n=%" PRIu64 ", but -n is %" PRIu64 "\n", g_prog, path.c_str(), fn, n);
    ok = false;
  }
  stride = hdr[0];
  if (ok) {
    deg.resize(n);
    ok = fread(deg.data(), 1, n, f) == n;
    const size_t pad = (4 - (n & 3)) & 3;
    char p[4];
    if (ok && pad) ok = fread(p, 1, pad, f) == pad;
    ids.resize(n * stride);
    if (ok) ok = fread(ids.data(), 4, n * stride, f) == n * stride;
  }
  fclose(f);
  if (!ok) fprintf(stderr, "%s: %s is not a valid peer table\n", g_prog, path.c_str());
  return ok;
}

// -payload / -pick / -every of a -rumors run.
struct BoundedSet {
  bool on = false;       // one of the three flags was given
  uint32_t payload = 0;  // rumors per message at most; 0: no cap
  uint32_t pick = GS_PICK_LOW;
  uint64_t every = 0;    // rumor j enters at round j * every
};

// -rumors R: R push-pull broadcasts from keyed senders in one pass (DESIGN.md
// section 4.9).  One gs_run per 10-ms poll, so that every poll's line can show
// the least-covered started rumor; then one line per rumor and the round at
// which all were covered.  A bounded set steps its ten rounds with gs_step
// instead, under which every round is a poll: a rumor's round of 99 % is then
// exact, as its rounds from start want it.  Without -payload it runs with a
// payload of 64, which moves what no cap moves and counts the traffic.
int run_rumor_set(gs_ctx* c, const gs_params& p, uint32_t R, uint64_t max_ticks, double ov_wall,
                  const BoundedSet& bs) {
  printf("=== Broadcast %u rumors ===\n", R);
  fflush(stdout);
  const auto b0 = std::chrono::steady_clock::now();
  int rc;
  if (bs.on) {
    rc = gs_rumorset_set_payload(c, bs.payload ? bs.payload : GS_RUMORSET_MAX, bs.pick);
    if (rc) return die(c, rc, "gs_rumorset_set_payload");
    std::vector<int64_t> senders(R, -1), starts(R);
    for (uint32_t j = 0; j < R; ++j) starts[j] = (int64_t)(j * bs.every);
    rc = gs_rumorset_begin_at(c, senders.data(), starts.data(), R);
    if (rc) return die(c, rc, "gs_rumorset_begin_at");
  } else {
    rc = gs_broadcast_begin(c, -1);  // every sender keyed
    if (rc) return die(c, rc, "gs_broadcast_begin");
  }
  std::vector<gs_rumor_stats> rs(R);
  size_t nrs = 0;
  int32_t status = GS_RUN_MAX_TICKS;
  gs_tick_stats tot{};
  do {
    gs_totals(c, &tot);
    if (bs.on) {
      rc = gs_step(c, (uint32_t)std::min<uint64_t>(10, max_ticks - std::min(tot.tick, max_ticks)), nullptr);
      if (rc) return die(c, rc, "gs_step");
    } else {
      rc = gs_run(c, 10, std::min<uint64_t>(tot.tick + 10, max_ticks), nullptr, 0, nullptr, &status);  // one poll
      if (rc) return die(c, rc, "gs_run");
    }
    rc = gs_rumorset_results(c, rs.data(), rs.size(), &nrs);
    if (rc) return die(c, rc, "gs_rumorset_results");
    gs_totals(c, &tot);
    uint64_t least = p.n;
    bool any = false;
    for (uint32_t j = 0; j < R; ++j)
      if (rs[j].started) {
        least = std::min<uint64_t>(least, rs[j].received);
        any = true;
      }
    if (bs.on) status = !any ? GS_RUN_QUIESCENT : tot.pending == 0 ? GS_RUN_COVERED : GS_RUN_MAX_TICKS;  // gs_run's rule
    char pb[64];
    gs_format_float32((any ? (float)least / (float)p.n : 0.0f) * 100.0f, pb, sizeof(pb));
    printf("%s%% covered, took %s\n", pb, dur_ms(tot.tick).c_str());
  } while (status == GS_RUN_MAX_TICKS && tot.tick < max_ticks);
  for (uint32_t j = 0; j < R; ++j) {
    printf("rumor %u: sender %" PRId64 ", %" PRIu64 " nodes, ", j, rs[j].sender, rs[j].received);
    if (bs.on) printf("start %s, ", dur_ms(j * bs.every).c_str());
    if (!rs[j].started) printf("never started (its sender is failed)\n");
    else if (rs[j].tick_99 && bs.on)
      printf("99%% after %s, %" PRIu64 " rounds from start\n", dur_ms(rs[j].tick_99).c_str(),
             rs[j].tick_99 - j * bs.every);
    else if (rs[j].tick_99) printf("99%% after %s\n", dur_ms(rs[j].tick_99).c_str());
    else printf("99%% not reached\n");
  }
  gs_rumorset_traffic tr{};
  if (bs.on) {
    rc = gs_rumorset_traffic_get(c, &tr);
    if (rc) return die(c, rc, "gs_rumorset_traffic_get");
  }
  const double bc_wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - b0).count();
  if (status != GS_RUN_COVERED) {
    fflush(stdout);
    fprintf(stderr, "%s: %s before every rumor reached 99%% coverage\n", g_prog,
            status == GS_RUN_QUIESCENT ? "no rumor started" : "-maxticks reached");
    gs_destroy(c);
    return 3;
  }
  printf("--- Took %s to get 99%% of all %u rumors ---\n\n", dur_ms(tot.tick).c_str(), R);
  printf("Total message %" PRIu64 " Total Crashed %" PRIu64 "\n", tot.messages, tot.crashed);
  if (bs.on)
    printf("Rumor copies wanted %" PRIu64 " carried %" PRIu64 ", messages bound by the payload %" PRIu64 "\n", tr.wanted,
           tr.carried, tr.bound);
  fflush(stdout);
  fprintf(stderr, "[gossip_sim] wall: overlay %.3f s, %u rumors %.3f s\n", ov_wall, R, bc_wall);
  gs_destroy(c);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  g_prog = argv[0];
  // simulator.go:187-193 (fanin's default is Fanout+1 evaluated before Parse: 6)
  g_flags = {
      {"n", "int", "total number of nodes", "50000", true, "50000"},
      {"fanout", "int", "fanout", "5", true, "5"},
      {"fanin", "int", "fanin", "6", true, "6"},
      {"delaylow", "int", "delay low (ms)", "10", true, "10"},
      {"delayhigh", "int", "delay high (ms)", "20", true, "20"},
      {"droprate", "float", "message drop rate", "0.1", true, "0.1"},
      {"crashrate", "float", "machine crash rate", "0.001", true, "0.001"},
      {"seed", "uint", "Philox key for every random decision", "1", false, "1"},
      {"trial", "uint", "Philox trial index", "0", false, "0"},
      {"trials", "int", "independent trials trial .. trial+trials-1 batched in one run (one line per trial)",
       "1", false, "1"},
      {"device", "int", "HIP device ordinal", "0", false, "0"},
      {"gpus", "int", "node-range shards over devices device .. device+gpus-1 (one process)", "1", false,
       "1"},
      {"peers", "string", "injected peer-table file (skips overlay construction)", "", false, ""},
      {"model", "string", "dissemination model: flood (the reference), pushpull, rumor or median (extensions)",
       "flood", false, "flood"},
      {"k", "int", "rumor model: a node stops calling after this many calls that reached an informed peer; "
       "median model: the counter steps and the rounds of the final phase, 1..127 (default there: "
       "ceil(log2 log2 n) + 1)",
       "2", false, "2"},
      {"batch", "int", "median model: this many independent trials trial .. trial+batch-1 in one batched context "
       "(gs_create_batch; one line per trial)", "0", false, "0"},
      {"packed", "bool", "with -batch: 16-bit tallies (GS_FLAG_MEDIAN_PACKED), so n may reach 50,304 on an MI355X; "
       "a table that names one node in more than 32,766 slots is refused", "false", false, "false"},
      {"blind", "bool", "rumor model: a hot node loses interest without waiting for a reply (GS_RUMOR_BLIND)",
       "false", false, "false"},
      {"coin", "bool", "rumor model: lose interest with probability 1/k per event, not after k events (GS_RUMOR_COIN)",
       "false", false, "false"},
      {"pull", "bool", "rumor model: every node calls and hot nodes answer (GS_RUMOR_PULL)", "false", false,
       "false"},
      {"rumors", "int", "pushpull model: this many rumors, 1..64, from keyed senders over one table in one pass "
       "(gs_create_rumorset; one line per rumor)", "0", false, "0"},
      {"payload", "int", "with -rumors: a message carries at most this many rumors, 1..64 (0: no cap; "
       "gs_rumorset_set_payload)", "0", false, "0"},
      {"pick", "string", "with -rumors: which wanted rumors a capped message carries: low (lowest indices, oldest "
       "first), high or rotate", "low", false, "low"},
      {"every", "int", "with -rumors: rumor j enters at round j * this (gs_rumorset_begin_at)", "0", false, "0"},
      {"maxticks", "int", "give up after this many simulated ms per phase", "10000000", false,
       "10000000"},
  };
  parse(argc, argv);
  // every flag is checked before the parameter echo and before any device call
  const std::string model = find("model")->val;
  if (model != "flood" && model != "pushpull" && model != "rumor" && model != "median") {
    fprintf(stderr, "invalid value \"%s\" for flag -model: want flood, pushpull or rumor, or median\n",
            model.c_str());
    return 2;
  }
  long long rumor_k = ival("k");
  if (model == "median" && !find("k")->given) {
    // The counter must outlast the spread, or B nodes whose partners are all done stay B (DESIGN.md
    // section 4.8): O(ln ln n) steps in the paper; ceil(log2 log2 n) + 1 here.
    const double l2 = std::log2(std::max<double>(4.0, (double)ival("n")));
    rumor_k = std::min<long long>(127, (long long)std::ceil(std::log2(l2)) + 1);
  }
  if (model == "rumor" && (rumor_k < 1 || rumor_k > 255)) {
    fprintf(stderr, "invalid value \"%s\" for flag -k: want 1..255\n", find("k")->val.c_str());
    usage();
    return 2;
  }
  if (model == "median" && (rumor_k < 1 || rumor_k > 127)) {
    fprintf(stderr, "invalid value \"%s\" for flag -k: -model median wants 1..127\n", find("k")->val.c_str());
    usage();
    return 2;
  }
  if (model == "median" && ival("trials") > 1) {
    fprintf(stderr, "flag -trials %s with -model median: the median-counter model runs one trial on one device "
            "(GS_MODEL_MEDIAN)\n", find("trials")->val.c_str());
    usage();
    return 2;
  }
  const bool median_batch = find("batch")->given;
  if (median_batch && model != "median") {
    fprintf(stderr, "flag -batch needs -model median (it runs a batch of median-counter trials)\n");
    usage();
    return 2;
  }
  if (median_batch && (ival("batch") < 1 || ival("batch") > 0x7FFFFFFFll)) {
    fprintf(stderr, "invalid value \"%s\" for flag -batch: want at least 1\n", find("batch")->val.c_str());
    usage();
    return 2;
  }
  if (median_batch && ival("gpus") > 1) {
    fprintf(stderr, "flag -batch with -gpus %s: a median batch runs on one device (GS_MODEL_MEDIAN)\n",
            find("gpus")->val.c_str());
    usage();
    return 2;
  }
  const bool median_packed = find("packed")->val == "true";
  if (median_packed && !median_batch) {
    fprintf(stderr, "flag -packed needs -batch (it packs the tallies of a batch of median-counter trials)\n");
    usage();
    return 2;
  }
  const bool rumor_set = find("rumors")->given;
  if (rumor_set && model != "pushpull") {
    fprintf(stderr, "flag -rumors needs -model pushpull (it runs concurrent push-pull rumors)\n");
    usage();
    return 2;
  }
  if (rumor_set && (ival("rumors") < 1 || ival("rumors") > (long long)GS_RUMORSET_MAX)) {
    fprintf(stderr, "invalid value \"%s\" for flag -rumors: want 1..64\n", find("rumors")->val.c_str());
    usage();
    return 2;
  }
  if (rumor_set && (ival("trials") > 1 || ival("gpus") > 1)) {
    fprintf(stderr, "flag -rumors with -trials or -gpus above 1: a rumor set runs one trial on one device\n");
    usage();
    return 2;
  }
  BoundedSet bs;
  for (const char* name : {"payload", "pick", "every"}) {
    if (!find(name)->given) continue;
    if (!rumor_set) {
      fprintf(stderr, "flag -%s needs -rumors (it bounds a rumor set)\n", name);
      usage();
      return 2;
    }
    bs.on = true;
  }
  if (bs.on) {
    const std::string pk = find("pick")->val;
    if (ival("payload") < 0 || ival("payload") > (long long)GS_RUMORSET_MAX) {
      fprintf(stderr, "invalid value \"%s\" for flag -payload: want 0..64\n", find("payload")->val.c_str());
      usage();
      return 2;
    }
    if (pk != "low" && pk != "high" && pk != "rotate") {
      fprintf(stderr, "invalid value \"%s\" for flag -pick: want low, high or rotate\n", pk.c_str());
      usage();
      return 2;
    }
    if (ival("every") < 0 || ival("every") * (ival("rumors") - 1) > 0x7FFFFFFFll || ival("every") > 0x7FFFFFFFll) {
      fprintf(stderr, "invalid value \"%s\" for flag -every: the last rumor's start must be a round below 2^31\n",
              find("every")->val.c_str());
      usage();
      return 2;
    }
    bs.payload = (uint32_t)ival("payload");
    bs.pick = pk == "high" ? GS_PICK_HIGH : pk == "rotate" ? GS_PICK_ROTATE : GS_PICK_LOW;
    bs.every = (uint64_t)ival("every");
  }

  uint32_t rumor_mode = 0;
  for (const auto& fb : {std::make_pair("blind", GS_RUMOR_BLIND), std::make_pair("coin", GS_RUMOR_COIN),
                         std::make_pair("pull", GS_RUMOR_PULL)}) {
    if (find(fb.first)->val != "true") continue;
    if (model != "rumor") {
      fprintf(stderr, "flag -%s needs -model rumor (it selects a variant of the rumor model)\n", fb.first);
      usage();
      return 2;
    }
    rumor_mode |= fb.second;
  }

  printf("=== Parameters ===\n");                              // :197-204
  {
    std::map<std::string, Flag*> sorted;
    for (auto& f : g_flags) if (f.echo) sorted[f.name] = &f;
    for (auto& kv : sorted) {
      printf("%s=%s", kv.first.c_str(), kv.second->val.c_str());
      if (kv.first == "delaylow" || kv.first == "delayhigh") printf("ms");
      printf("\n");
    }
  }
  fflush(stdout);

  gs_params p{};
  p.n = (uint64_t)ival("n");
  p.fanout = (int32_t)ival("fanout");
  p.fanin = (int32_t)ival("fanin");
  p.delay_low = (int32_t)ival("delaylow");
  p.delay_high = (int32_t)ival("delayhigh");
  p.drop_rate = fval("droprate");
  p.crash_rate = fval("crashrate");
  p.seed = strtoull(find("seed")->val.c_str(), nullptr, 10);
  p.trial = (uint32_t)strtoull(find("trial")->val.c_str(), nullptr, 10);
  p.device = (int32_t)ival("device");
  p.model = model == "pushpull" ? GS_MODEL_PUSHPULL
            : model == "rumor"  ? GS_MODEL_RUMOR
            : model == "median" ? GS_MODEL_MEDIAN
                                : GS_MODEL_FLOOD;
  if (p.model == GS_MODEL_MEDIAN) p.rumor_k = (uint32_t)rumor_k;
  if (median_packed) p.flags |= GS_FLAG_MEDIAN_PACKED;
  const bool self_ending = p.model == GS_MODEL_RUMOR || p.model == GS_MODEL_MEDIAN;  // runs to its own end
  if (p.model == GS_MODEL_RUMOR) {
    p.rumor_k = (uint32_t)rumor_k;
    p.rumor_mode = rumor_mode;
  }
  const uint64_t max_ticks = (uint64_t)ival("maxticks");
  const long long ntrials = median_batch ? ival("batch") : ival("trials");
  if (ntrials < 1 || ntrials > 0x7FFFFFFFll) {
    fprintf(stderr, "invalid value \"%s\" for flag -trials: want at least 1\n", find("trials")->val.c_str());
    usage();
    return 2;
  }
  p.trials = (uint32_t)ntrials;
  if (ival("n") <= 0) {
    fprintf(stderr, "panic: invalid argument to Intn\n");  // simulator.go:240 with N=0
    return 2;
  }
  gs_ctx* c = nullptr;
  int rc;
  const int64_t gpus = ival("gpus");
  if (gpus > 1) {
    std::vector<int> devs;
    for (int64_t i = 0; i < gpus; ++i) devs.push_back((int)(p.device + i));
    rc = gs_create_multi(&p, devs.data(), (int)gpus, &c);
  } else if (p.model == GS_MODEL_RUMOR && p.trials > 1) {
    rc = gs_create_trials(&p, &c);  // gs_create keeps refusing the combination
  } else if (median_batch) {
    rc = gs_create_batch(&p, &c);  // the other creates keep refusing a median batch
  } else if (rumor_set) {
    rc = gs_create_rumorset(&p, (uint32_t)ival("rumors"), &c);  // the only way in to a rumor set
  } else {
    rc = gs_create(&p, &c);
  }
  if (rc) {
    fprintf(stderr, "%s: gs_create failed: %s (%s)\n", g_prog, gs_strerror(rc), gs_last_error(nullptr));
    return 1;
  }

  printf("\n=== Constructing Overlay ===\n");                   // :219
  const auto w0 = std::chrono::steady_clock::now();
  const std::string peers = find("peers")->val;
  uint64_t stab = 0;
  if (!peers.empty() && p.trials > 1) {
    fprintf(stderr, "%s: -peers holds one table; -trials > 1 builds every trial's overlay\n", g_prog);
    gs_destroy(c);
    return 2;
  }
  if (!peers.empty()) {
    std::vector<uint8_t> deg;
    std::vector<uint32_t> ids;
    uint32_t stride = 0;
    if (!load_peers_file(peers, p.n, deg, ids, stride)) { gs_destroy(c); return 1; }
    rc = gs_load_peers(c, deg.data(), ids.data(), stride);
    if (rc) return die(c, rc, "gs_load_peers");
    stab = 10;  // one empty poll window: nothing to construct
  } else {
    std::vector<gs_window> win(1 << 16);
    size_t nwin = 0;
    rc = gs_build_overlay(c, max_ticks, win.data(), win.size(), &nwin, &stab);
    if (rc) return die(c, rc, "gs_build_overlay");
    for (size_t i = 0; i < nwin && i < win.size(); ++i)     // :230
      printf("break %" PRIu64 " makeup %" PRIu64 " elasped %s\n", win[i].breakups, win[i].makeups,
             dur_ms(win[i].tick).c_str());
  }
  printf("--- Took %s to stabilize ---\n\n", dur_ms(stab).c_str()); // :235
  const double ov_wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count();

  if (rumor_set) return run_rumor_set(c, p, (uint32_t)ival("rumors"), max_ticks, ov_wall, bs);
  printf("=== Broadcast one message ===\n");                    // :237
  fflush(stdout);
  const auto b0 = std::chrono::steady_clock::now();
  rc = gs_broadcast_begin(c, -1);                               // :239-241
  if (rc) return die(c, rc, "gs_broadcast_begin");
  // gs_run is the poll loop (:243-251) with the engine's stop rule: one row
  // per 10-ms poll, printed in the reference's format
  std::vector<gs_tick_stats> polls((size_t)std::min<uint64_t>(max_ticks / 10 + 2, 1u << 20));
  size_t npoll = 0;
  int32_t status = GS_RUN_MAX_TICKS;
  rc = gs_run(c, 10, max_ticks, polls.data(), polls.size(), &npoll, &status);
  if (rc) return die(c, rc, "gs_run");
  if (p.trials > 1) {  // one line per trial: its figures at its own stopping poll (gs_trial_results)
    std::vector<gs_trial_stats> tr(p.trials);
    size_t ntr = 0;
    rc = gs_trial_results(c, tr.data(), tr.size(), &ntr);
    if (rc) return die(c, rc, "gs_trial_results");
    uint32_t got99 = 0;
    if (p.model == GS_MODEL_RUMOR || median_batch) {  // the model's own outputs per trial, then their statistics
      static const char* const names[] = {"covered", "quiescent", "maxticks"};
      const size_t T = std::min(ntr, tr.size());
      // a median batch: the stranded nodes, those still active (B or C) at the trial's stop.  A trial
      // that ended by itself has none and gets none later, and the others all stop at the run's last
      // poll, so the state bytes at the end of the run give every trial's count.
      std::vector<uint64_t> stranded(T, 0);
      if (median_batch) {
        std::vector<uint8_t> stb((size_t)p.trials * p.n);
        rc = gs_read_median_state(c, stb.data(), stb.size());
        if (rc) return die(c, rc, "gs_read_median_state");
        for (size_t i = 0; i < T; ++i)
          for (uint64_t v = 0; v < p.n; ++v) {
            const uint8_t b = stb[i * p.n + v];
            stranded[i] += b != 0 && b != 255;
          }
      }
      const int F = median_batch ? 4 : 3;
      double sum[4] = {0, 0, 0, 0}, sq[4] = {0, 0, 0, 0};
      uint32_t ended = 0;
      auto figures = [&](size_t i, double* x) {
        x[0] = 1.0 - (double)tr[i].received / (double)p.n;
        x[1] = (double)tr[i].messages / (double)p.n;
        x[2] = (double)tr[i].tick;
        x[3] = (double)stranded[i];
      };
      for (size_t i = 0; i < T; ++i) {
        char rb[64], mb[64];
        gs_format_float32(1.0f - (float)tr[i].received / (float)p.n, rb, sizeof(rb));
        gs_format_float32((float)tr[i].messages / (float)p.n, mb, sizeof(mb));
        printf("trial %" PRIu64 ": Residue %s, %s messages per node after %s, %s", tr[i].trial, rb, mb,
               dur_ms(tr[i].tick).c_str(), names[tr[i].status >= 0 && tr[i].status <= 2 ? tr[i].status : 2]);
        if (median_batch) printf(", stranded %" PRIu64, stranded[i]);
        printf("\n");
        double x[4];
        figures(i, x);
        for (int f = 0; f < F; ++f) sum[f] += x[f];
        if (tr[i].status != GS_RUN_MAX_TICKS) ++ended;
      }
      double mean[4], sd[4];
      for (int f = 0; f < F; ++f) mean[f] = T ? sum[f] / (double)T : 0.0;
      for (size_t i = 0; i < T; ++i) {  // two passes: the deviations from the mean
        double x[4];
        figures(i, x);
        for (int f = 0; f < F; ++f) sq[f] += (x[f] - mean[f]) * (x[f] - mean[f]);
      }
      for (int f = 0; f < F; ++f) sd[f] = T > 1 ? std::sqrt(sq[f] / (double)(T - 1)) : 0.0;
      printf("--- %zu trials: residue mean %s sd %s, messages per node mean %s sd %s, rounds mean %s sd %s", T,
             gofloat(mean[0]).c_str(), gofloat(sd[0]).c_str(), gofloat(mean[1]).c_str(), gofloat(sd[1]).c_str(),
             gofloat(mean[2]).c_str(), gofloat(sd[2]).c_str());
      if (median_batch) printf(", stranded mean %s sd %s", gofloat(mean[3]).c_str(), gofloat(sd[3]).c_str());
      printf(" ---\n");
      fflush(stdout);
      const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - b0).count();
      fprintf(stderr, "[gossip_sim] wall: overlay %.3f s, %u broadcasts %.3f s\n", ov_wall, p.trials, wall);
      gs_destroy(c);
      return ended == T ? 0 : 3;
    }
    for (size_t i = 0; i < ntr && i < tr.size(); ++i) {
      const float percent = (float)tr[i].received / (float)p.n;
      char pb[64];
      gs_format_float32(percent * 100.0f, pb, sizeof(pb));
      printf("trial %" PRIu64 ": %s%% covered, took %s, Total message %" PRIu64 " Total Crashed %" PRIu64 "\n",
             tr[i].trial, pb, dur_ms(tr[i].tick).c_str(), tr[i].messages, tr[i].crashed);
      if (tr[i].status == GS_RUN_COVERED) ++got99;
    }
    printf("--- %u of %u trials got 99%% ---\n", got99, p.trials);
    fflush(stdout);
    const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - b0).count();
    fprintf(stderr, "[gossip_sim] wall: overlay %.3f s, %u broadcasts %.3f s\n", ov_wall, p.trials, wall);
    gs_destroy(c);
    return got99 == p.trials ? 0 : 3;
  }
  for (size_t i = 0; i < npoll && i < polls.size(); ++i) {
    const float percent = (float)polls[i].received / (float)p.n;
    char pb[64];
    gs_format_float32(percent * 100.0f, pb, sizeof(pb));
    printf("%s%% covered, took %s\n", pb, dur_ms(polls[i].tick).c_str());
  }
  gs_tick_stats tot{};
  gs_totals(c, &tot);
  const double bc_wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - b0).count();
  if (self_ending) {  // the model's own outputs, at quiescence
    char rb[64], mb[64];
    gs_format_float32(1.0f - (float)tot.received / (float)p.n, rb, sizeof(rb));
    gs_format_float32((float)tot.messages / (float)p.n, mb, sizeof(mb));
    printf("--- Residue %s, %s messages per node after %s ---\n", rb, mb, dur_ms(tot.tick).c_str());
    if (status == GS_RUN_QUIESCENT) {  // the model's normal end: it fell quiet below 99 %
      printf("\nTotal message %" PRIu64 " Total Crashed %" PRIu64 "\n", tot.messages, tot.crashed);
      fflush(stdout);
      fprintf(stderr, "[gossip_sim] wall: overlay %.3f s, broadcast %.3f s\n", ov_wall, bc_wall);
      gs_destroy(c);
      return 0;
    }
  }
  if (status != GS_RUN_COVERED) {
    fflush(stdout);
    fprintf(stderr, "%s: %s before 99%% coverage (the reference would poll forever)\n", g_prog,
            status == GS_RUN_QUIESCENT ? "no broadcast left in flight" : "-maxticks reached");
    gs_destroy(c);
    return 3;
  }
  uint64_t t99 = tot.tick;
  if (self_ending) {  // the run went on to quiescence: the first covered poll
    gs_trial_stats tr{};
    size_t ntr = 0;
    if (gs_trial_results(c, &tr, 1, &ntr) == GS_OK && ntr == 1 && tr.tick_99) t99 = tr.tick_99;
  }
  printf("--- Took %s to get 99%% ---\n\n", dur_ms(t99).c_str());  // :252
  printf("Total message %" PRIu64 " Total Crashed %" PRIu64 "\n", tot.messages, tot.crashed); // :253
  fflush(stdout);
  fprintf(stderr,
          "[gossip_sim] wall: overlay %.3f s, broadcast %.3f s; %" PRIu64
          " delivered sends -> %.3e msgs/s\n",
          ov_wall, bc_wall, tot.sent, bc_wall > 0 ? (double)tot.sent / bc_wall : 0.0);
  gs_destroy(c);
  return 0;
}
