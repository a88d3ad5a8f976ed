// devmem_harness.cpp -- the device-block cache (gs_devmem.cpp) and the
// reverse-table pass planner (gs_rev_plan.h) against plain models, on the CPU.
//
// This program is linked with the product's gs_devmem.cpp, unchanged, and
// defines the eight HIP entry points that file calls itself: a fake driver
// with several devices, a capacity per device, a table of live allocations and
// a log of every call.  Nothing backs the addresses it hands out; they come
// from a high range and are never reused, so a stale address cannot alias a
// new block.
//
//   devmem_harness <scenario>      one JSON line; exit status 1 on a violated check
//
// The process reads GS_DEVMEM_CACHE and GS_DEVMEM_POISON once, so every
// scenario is a fresh process (tests/test_devmem_model.py).
//
// The model (struct Sim) is written from the contract in gs_devmem.h and the
// header comment of gs_devmem.cpp, not from the allocator's code: a flat list
// of extents per slab and linear scans.  Before every request it predicts the
// class of the outcome (plain hipMalloc; a cache hit and the size of the extent
// taken; a new slab; which slabs go back to the driver first; failure), and
// after the call it takes the address the allocator chose (ties between equal
// extents are the allocator's) and checks everything else.
#include "gs_devmem.h"
#include "gs_rev_plan.h"

#include <algorithm>
#include <atomic>
#include <cinttypes>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <random>
#include <string>
#include <thread>
#include <vector>

namespace {

constexpr size_t MiB = 1ull << 20, GiB = 1ull << 30;
// the contract's numbers (gs_devmem.h)
constexpr size_t kMin = 64 * MiB;    // smaller requests bypass the cache
constexpr size_t kGran = 2 * MiB;    // cached requests are rounded up to this
constexpr size_t kMargin = 8 * GiB;  // device memory left beside the cache
constexpr size_t kDeviceBytes = 288ull * 1000 * 1000 * 1000;
constexpr int kDevices = 3;

std::string g_scenario, g_ctx;

[[noreturn]] void fail(int line, const char* what, const char* fmt, ...) {
  char buf[512] = "";
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  printf("{\"scenario\": \"%s\", \"ok\": false, \"line\": %d, \"check\": \"%s\", \"detail\": \"%s\", \"at\": \"%s\"}\n",
         g_scenario.c_str(), line, what, buf, g_ctx.c_str());
  fflush(stdout);
  _Exit(1);
}
#define CHECK(c, ...)                                 \
  do {                                                \
    if (!(c)) fail(__LINE__, #c, "" __VA_ARGS__);     \
  } while (0)

// ---------------------------------------------------------------- fake driver
struct Call {
  char kind;  // M hipMalloc, F hipFree, Y hipDeviceSynchronize, S hipSetDevice, I hipMemGetInfo, Z hipMemset
  int dev;    // the calling thread's current device (S: the new one)
  uintptr_t addr;
  size_t size;
  hipError_t err;
  int value = 0;  // Z: the byte
};
struct Alloc {
  size_t size;
  int dev;
};
struct Fake {
  std::mutex mu;
  size_t capacity[kDevices];
  size_t live_bytes[kDevices] = {};
  std::map<uintptr_t, Alloc> live;
  std::map<uintptr_t, size_t> blocks;  // blocks the harness holds (registered by it): a slab with one is never freed
  std::vector<Call> log;
  uintptr_t next = 0x700000000000ull;
  bool contiguous = false;  // place the next allocations back to back
  int fail_next = 0;        // fail that many hipMallocs whatever the room (fragmentation)
  int fail_fill = 0;        // fail that many hipMemsets
  uint64_t n_malloc = 0, n_free = 0, unknown_free = 0, freed_under_block = 0;
  Fake() {
    for (size_t& c : capacity) c = kDeviceBytes;
  }
};
Fake& fk() {
  static Fake* f = new Fake;
  return *f;
}
thread_local int t_dev = 0;  // the current device is per thread, as in HIP

}  // namespace

extern "C" {
hipError_t hipMalloc(void** p, size_t size) {
  Fake& f = fk();
  std::lock_guard<std::mutex> g(f.mu);
  ++f.n_malloc;
  const int d = t_dev;
  const bool injected = f.fail_next > 0;
  if (injected) --f.fail_next;
  if (injected || f.live_bytes[d] + size > f.capacity[d]) {
    f.log.push_back({'M', d, 0, size, hipErrorOutOfMemory});
    return hipErrorOutOfMemory;
  }
  const uintptr_t a = f.next;
  f.next += ((size + kGran - 1) & ~(kGran - 1)) + (f.contiguous ? 0 : kGran);
  f.live[a] = {size, d};
  f.live_bytes[d] += size;
  f.log.push_back({'M', d, a, size, hipSuccess});
  *p = (void*)a;
  return hipSuccess;
}
hipError_t hipFree(void* p) {
  Fake& f = fk();
  std::lock_guard<std::mutex> g(f.mu);
  ++f.n_free;
  if (!p) return hipSuccess;
  const uintptr_t a = (uintptr_t)p;
  auto it = f.live.find(a);
  if (it == f.live.end()) {
    ++f.unknown_free;
    f.log.push_back({'F', t_dev, a, 0, hipErrorInvalidValue});
    return hipErrorInvalidValue;
  }
  auto b = f.blocks.lower_bound(a);
  if (b != f.blocks.end() && b->first < a + it->second.size) ++f.freed_under_block;
  f.live_bytes[it->second.dev] -= it->second.size;
  f.log.push_back({'F', t_dev, a, it->second.size, hipSuccess});
  f.live.erase(it);
  return hipSuccess;
}
hipError_t hipGetDevice(int* d) {
  *d = t_dev;
  return hipSuccess;
}
hipError_t hipSetDevice(int d) {
  if (d < 0 || d >= kDevices) return hipErrorInvalidDevice;
  t_dev = d;
  Fake& f = fk();
  std::lock_guard<std::mutex> g(f.mu);
  f.log.push_back({'S', d, 0, 0, hipSuccess});
  return hipSuccess;
}
hipError_t hipMemGetInfo(size_t* freeb, size_t* total) {
  Fake& f = fk();
  std::lock_guard<std::mutex> g(f.mu);
  *total = f.capacity[t_dev];
  *freeb = f.capacity[t_dev] > f.live_bytes[t_dev] ? f.capacity[t_dev] - f.live_bytes[t_dev] : 0;
  f.log.push_back({'I', t_dev, 0, *freeb, hipSuccess});
  return hipSuccess;
}
hipError_t hipDeviceSynchronize(void) {
  Fake& f = fk();
  std::lock_guard<std::mutex> g(f.mu);
  f.log.push_back({'Y', t_dev, 0, 0, hipSuccess});
  return hipSuccess;
}
hipError_t hipMemset(void* p, int value, size_t size) {
  Fake& f = fk();
  std::lock_guard<std::mutex> g(f.mu);
  const bool injected = f.fail_fill > 0;
  if (injected) --f.fail_fill;
  const hipError_t e = injected ? hipErrorLaunchFailure : hipSuccess;
  f.log.push_back({'Z', t_dev, (uintptr_t)p, size, e, value});
  return e;
}
hipError_t hipGetLastError(void) { return hipSuccess; }
}

namespace {

bool cache_enabled() {
  const char* s = getenv("GS_DEVMEM_CACHE");
  return !(s && atoi(s) == 0);
}
size_t round_up(size_t b) { return (b + kGran - 1) / kGran * kGran; }
// GS_DEVMEM_POISON as DESIGN.md section 9.1 documents it: decimal or 0x.., 1..255, else off
// (the out-of-range and malformed values are pinned from outside, by tests/test_devmem_model.py)
int poison_byte() {
  const char* s = getenv("GS_DEVMEM_POISON");
  if (!s || !*s) return 0;
  char* end = nullptr;
  const long v = strtol(s, &end, 0);
  return (*end || v < 1 || v > 255) ? 0 : (int)v;
}

// ------------------------------------------------------------------ the model
enum Cls { PLAIN, PLAIN_FAIL, HIT, NEW_SLAB, FAIL };
const char* cls_name[] = {"plain", "plain_fail", "hit", "new_slab", "fail"};

struct Outcome {
  Cls cls = FAIL;
  size_t ext_size = 0;          // HIT: the size of the extent taken (before the split)
  std::vector<size_t> trimmed;  // sizes of the slabs returned to the driver, ascending
  int mallocs = 0;              // hipMalloc calls
  bool relaxed = false;         // HIT only after a hipMalloc failed
  uintptr_t addr = 0;
  hipError_t err = hipSuccess;
  size_t trimmed_bytes() const {
    size_t s = 0;
    for (size_t t : trimmed) s += t;
    return s;
  }
};

struct MExt {
  uintptr_t addr;
  size_t size;
  bool used;
};
struct MSlab {
  uintptr_t base;
  size_t size;
  int dev;
  std::vector<MExt> ext;  // in address order, covering the slab
  bool all_free() const { return ext.size() == 1 && !ext[0].used; }
};
struct Block {
  uintptr_t addr;
  size_t bytes;
  int dev;
  bool cached;
};

struct Sim {
  const bool enabled = cache_enabled();
  const int poison = poison_byte();
  std::vector<MSlab> slabs;
  std::vector<Block> blocks;  // live, handed out
  uint64_t hits = 0;
  int cur = 0;
  std::map<std::string, uint64_t> seen;  // outcome classes met, for the report

  // ---- model queries (linear scans)
  size_t dev_free(int d) const {
    size_t used = 0;
    for (const MSlab& s : slabs)
      if (s.dev == d) used += s.size;
    for (const Block& b : blocks)
      if (b.dev == d && !b.cached) used += b.bytes;
    Fake& f = fk();
    return f.capacity[d] > used ? f.capacity[d] - used : 0;
  }
  // free extents of device d: those of fully free slabs (interchangeable when
  // equal) and those beside a used extent
  void free_extents(int d, std::vector<size_t>& whole, std::vector<size_t>& part) const {
    for (const MSlab& s : slabs) {
      if (s.dev != d) continue;
      if (s.all_free())
        whole.push_back(s.size);
      else
        for (const MExt& x : s.ext)
          if (!x.used) part.push_back(x.size);
    }
  }
  static size_t best_fit(const std::vector<size_t>& whole, const std::vector<size_t>& part, size_t need) {
    size_t best = 0;
    for (const auto* v : {&whole, &part})
      for (size_t s : *v)
        if (s >= need && (!best || s < best)) best = s;
    return best;
  }
  // "as few bytes back to the driver as the request needs": the smallest
  // single free slab that covers `want`, else the largest first until covered
  static std::vector<size_t> choose_trim(std::vector<size_t>& whole, size_t want) {
    std::vector<size_t> out;
    std::sort(whole.begin(), whole.end());
    for (size_t i = 0; i < whole.size(); ++i)
      if (whole[i] >= want) {
        out.push_back(whole[i]);
        whole.erase(whole.begin() + i);
        return out;
      }
    size_t got = 0;
    while (!whole.empty() && got < want) {
      got += whole.back();
      out.push_back(whole.back());
      whole.pop_back();
    }
    return out;
  }
  size_t predict_largest(int d) const {
    size_t best = 0;
    const size_t f = dev_free(d);
    if (f > kMargin) {
      best = f - kMargin;
      // a cached-size request is rounded up, and the rounded block must fit
      if (enabled && best >= kMin) best = best / kGran * kGran;
    }
    if (enabled) {
      std::vector<size_t> whole, part;
      free_extents(d, whole, part);
      for (const auto* v : {&whole, &part})
        for (size_t s : *v) best = std::max(best, s);
    }
    return best;
  }

  Outcome predict_malloc(int d, size_t bytes) const {
    Outcome o;
    int inject = fk().fail_next;
    auto driver_gives = [&](size_t room, size_t want) {
      ++o.mallocs;
      if (inject > 0) {
        --inject;
        return false;
      }
      return room >= want;
    };
    if (!enabled || bytes < kMin) {
      o.cls = driver_gives(dev_free(d), bytes) ? PLAIN : PLAIN_FAIL;
      return o;
    }
    const size_t need = round_up(bytes);
    std::vector<size_t> whole, part;
    free_extents(d, whole, part);
    size_t s = best_fit(whole, part, need);
    // the best fit serves the request unless it is far too big for it
    if (s && !(s > 4 * need && s - need > GiB)) {
      o.cls = HIT;
      o.ext_size = s;
      return o;
    }
    // a new slab, with the margin beside it: make the room first
    size_t room = dev_free(d);
    if (room < need + kMargin) {
      o.trimmed = choose_trim(whole, need + kMargin - room);
      room += o.trimmed_bytes();
    }
    if (driver_gives(room, need)) {
      o.cls = NEW_SLAB;
    } else if ((s = best_fit(whole, part, need))) {  // no room: any extent that fits
      o.cls = HIT;
      o.relaxed = true;
      o.ext_size = s;
    } else if (whole.empty()) {
      o.cls = FAIL;
    } else {  // every free slab back to the driver and one more try
      for (size_t w : whole) {
        o.trimmed.push_back(w);
        room += w;
      }
      o.cls = driver_gives(room, need) ? NEW_SLAB : FAIL;
    }
    std::sort(o.trimmed.begin(), o.trimmed.end());
    return o;
  }

  // ---- applying what the allocator did
  struct LogView {
    int mallocs = 0, syncs = 0;
    std::vector<Call> frees, ok_mallocs, all_mallocs, sync_calls, fills, all;
  };
  static LogView since(size_t mark) {
    Fake& f = fk();
    std::lock_guard<std::mutex> g(f.mu);
    LogView v;
    for (size_t i = mark; i < f.log.size(); ++i) {
      const Call& c = f.log[i];
      v.all.push_back(c);
      if (c.kind == 'Z') v.fills.push_back(c);
      if (c.kind == 'M') {
        ++v.mallocs;
        v.all_mallocs.push_back(c);
        if (c.err == hipSuccess) v.ok_mallocs.push_back(c);
      } else if (c.kind == 'F') {
        v.frees.push_back(c);
      } else if (c.kind == 'Y') {
        ++v.syncs;
        v.sync_calls.push_back(c);
      }
    }
    return v;
  }
  static size_t mark() {
    Fake& f = fk();
    std::lock_guard<std::mutex> g(f.mu);
    return f.log.size();
  }
  // the slabs the driver got back: each a fully free slab of `d` (-1: any);
  // their sizes are what the model said
  void apply_trims(const std::vector<Call>& frees, int d, const std::vector<size_t>& predicted) {
    std::vector<size_t> got;
    for (const Call& c : frees) {
      CHECK(c.err == hipSuccess, "hipFree of %#zx failed", (size_t)c.addr);
      auto it = std::find_if(slabs.begin(), slabs.end(), [&](const MSlab& s) { return s.base == c.addr; });
      CHECK(it != slabs.end(), "hipFree of %#zx: not a slab's base", (size_t)c.addr);
      CHECK(it->all_free(), "hipFree of a slab with a live block or an uncoalesced extent");
      CHECK(d < 0 || it->dev == d, "slab of device %d trimmed for device %d", it->dev, d);
      got.push_back(it->size);
      slabs.erase(it);
    }
    std::sort(got.begin(), got.end());
    CHECK(got == predicted, "trimmed %zu slab(s), model says %zu", got.size(), predicted.size());
  }
  void reg(uintptr_t a, size_t n) {
    Fake& f = fk();
    std::lock_guard<std::mutex> g(f.mu);
    f.blocks[a] = n;
  }
  void unreg(uintptr_t a) {
    Fake& f = fk();
    std::lock_guard<std::mutex> g(f.mu);
    f.blocks.erase(a);
  }

  Outcome malloc(size_t bytes) {
    const int d = cur;
    Outcome o = predict_malloc(d, bytes);
    const size_t m = mark();
    void* p = nullptr;
    o.err = gs_dev_malloc(&p, bytes);
    o.addr = (uintptr_t)p;
    const LogView v = since(m);
    CHECK(v.mallocs == o.mallocs, "%d hipMalloc calls, model says %d (%s)", v.mallocs, o.mallocs, cls_name[o.cls]);
    const size_t need = round_up(bytes);
    const bool cached = enabled && bytes >= kMin;
    for (const Call& c : v.all_mallocs) CHECK(c.size == (cached ? need : bytes) && c.dev == d, "hipMalloc size/device");
    apply_trims(v.frees, d, o.trimmed);
    // the poison switch: off, the driver sees no fill; on, a block handed out
    // was filled whole with the byte and the device synchronised, as the last
    // two driver calls of the request
    if (!poison || o.err != hipSuccess) {
      CHECK(v.fills.empty(), "%zu fill(s) %s", v.fills.size(), poison ? "of a failed request" : "with the switch off");
    } else {
      CHECK(v.fills.size() == 1, "%zu fills of one block", v.fills.size());
      const Call& z = v.fills[0];
      CHECK(z.addr == o.addr && z.size == (cached ? need : bytes) && z.value == poison && z.dev == d,
            "fill of %zu bytes at %#zx with %d", z.size, (size_t)z.addr, z.value);
      const size_t k = v.all.size();
      CHECK(k >= 2 && v.all[k - 2].kind == 'Z' && v.all[k - 1].kind == 'Y' && v.all[k - 1].dev == d,
            "the fill and one sync do not end the request");
      CHECK(v.syncs == 1, "%d syncs after one fill", v.syncs);
    }
    switch (o.cls) {
      case PLAIN:
        CHECK(o.err == hipSuccess && v.ok_mallocs.size() == 1 && v.ok_mallocs[0].addr == o.addr);
        blocks.push_back({o.addr, bytes, d, false});
        break;
      case PLAIN_FAIL:
      case FAIL:
        CHECK(o.err == hipErrorOutOfMemory && !p && v.ok_mallocs.empty(), "expected failure, err %d", (int)o.err);
        break;
      case NEW_SLAB: {
        CHECK(o.err == hipSuccess && v.ok_mallocs.size() == 1 && v.ok_mallocs[0].addr == o.addr, "expected a new slab");
        slabs.push_back({o.addr, need, d, {{o.addr, need, true}}});
        blocks.push_back({o.addr, bytes, d, true});
        break;
      }
      case HIT: {
        CHECK(o.err == hipSuccess && v.ok_mallocs.empty(), "expected a cache hit");
        MExt* x = nullptr;
        MSlab* sl = nullptr;
        for (MSlab& s : slabs)
          for (MExt& e : s.ext)
            if (e.addr == o.addr) x = &e, sl = &s;
        CHECK(x && !x->used, "the block %#zx does not start a free extent", (size_t)o.addr);
        CHECK(sl->dev == d, "a request on device %d served from device %d", d, sl->dev);
        CHECK(x->size == o.ext_size, "extent of %zu taken, model says %zu", x->size, o.ext_size);
        CHECK((o.addr - sl->base) % kGran == 0);
        const size_t rest = x->size - need;
        x->used = true;
        x->size = need;
        if (rest) {
          const size_t i = x - sl->ext.data();
          sl->ext.insert(sl->ext.begin() + i + 1, MExt{o.addr + need, rest, false});
        }
        ++hits;
        blocks.push_back({o.addr, bytes, d, true});
        break;
      }
    }
    if (o.err == hipSuccess) reg(o.addr, cached ? need : bytes);
    std::string key = cls_name[o.cls];
    if (o.relaxed) key += "_relaxed";
    if (!o.trimmed.empty()) key += "_after_trim";
    ++seen[key];
    check_all();
    return o;
  }

  // a request whose fill fails: the fill's error, no block, and the books as
  // they were -- but for a slab mapped for it, which stays cached
  Outcome malloc_fill_fails(size_t bytes) {
    CHECK(poison, "this needs GS_DEVMEM_POISON");
    const int d = cur;
    Outcome o = predict_malloc(d, bytes);
    CHECK(o.cls == PLAIN || o.cls == HIT || o.cls == NEW_SLAB);
    DevMemStats a, b;
    gs_devmem_stats(&a);
    size_t live_before;
    {
      std::lock_guard<std::mutex> g(fk().mu);
      live_before = fk().live.size();
      fk().fail_fill = 1;
    }
    const size_t m = mark();
    void* p = (void*)16;
    o.err = gs_dev_malloc(&p, bytes);
    const LogView v = since(m);
    CHECK(o.err == hipErrorLaunchFailure && !p, "a failed fill returned %d and %p", (int)o.err, p);
    CHECK(v.fills.size() == 1 && v.fills[0].err != hipSuccess && v.mallocs == o.mallocs);
    gs_devmem_stats(&b);
    CHECK(b.hip_allocs == a.hip_allocs + (uint64_t)o.mallocs && b.cache_hits == a.cache_hits);
    const size_t need = round_up(bytes);
    if (o.cls == PLAIN) {  // the block went back to the driver
      CHECK(v.frees.size() == 1 && v.frees[0].addr == v.ok_mallocs[0].addr && v.frees[0].err == hipSuccess);
      CHECK(b.cached_bytes == a.cached_bytes && b.mapped_bytes == a.mapped_bytes);
    } else if (o.cls == HIT) {  // the extent is free again and merged as before
      CHECK(v.frees.empty() && b.cached_bytes == a.cached_bytes && b.mapped_bytes == a.mapped_bytes);
    } else {  // the new slab is a free cached extent
      CHECK(v.frees.empty() && v.ok_mallocs.size() == 1);
      CHECK(b.mapped_bytes == a.mapped_bytes + need && b.cached_bytes == a.cached_bytes + need);
      const uintptr_t base = v.ok_mallocs[0].addr;
      slabs.push_back({base, need, d, {{base, need, false}}});
    }
    std::lock_guard<std::mutex> g(fk().mu);
    CHECK(fk().live.size() == live_before + (o.cls == NEW_SLAB));
    return o;
  }

  // free of a live block; returns the slabs the headroom rule sent back
  Outcome free(uintptr_t addr) {
    auto bi = std::find_if(blocks.begin(), blocks.end(), [&](const Block& b) { return b.addr == addr; });
    CHECK(bi != blocks.end());
    const Block b = *bi;
    blocks.erase(bi);
    unreg(addr);
    Outcome o;
    if (b.cached) {
      MSlab* sl = nullptr;
      for (MSlab& s : slabs)
        if (addr >= s.base && addr < s.base + s.size) sl = &s;
      CHECK(sl);
      for (MExt& e : sl->ext)
        if (e.addr == addr) e.used = false;
      for (size_t i = 0; i + 1 < sl->ext.size();)  // free neighbours become one extent
        if (!sl->ext[i].used && !sl->ext[i + 1].used) {
          sl->ext[i].size += sl->ext[i + 1].size;
          sl->ext.erase(sl->ext.begin() + i + 1);
        } else {
          ++i;
        }
      const size_t room = dev_free(b.dev);
      if (room < kMargin) {
        std::vector<size_t> whole, part;
        free_extents(b.dev, whole, part);
        o.trimmed = choose_trim(whole, kMargin - room);
        std::sort(o.trimmed.begin(), o.trimmed.end());
      }
    }
    const size_t m = mark();
    o.err = gs_dev_free((void*)addr);
    const LogView v = since(m);
    CHECK(o.err == hipSuccess, "free of a live block: %d", (int)o.err);
    CHECK(v.mallocs == 0);
    if (b.cached) {
      // hipFree's contract: the block's device went idle first
      CHECK(v.syncs == 1 && v.sync_calls[0].dev == b.dev, "no hipDeviceSynchronize on the block's device");
      apply_trims(v.frees, b.dev, o.trimmed);
      if (!o.trimmed.empty()) ++seen["free_headroom_trim"];
    } else {
      CHECK(v.frees.size() == 1 && v.frees[0].addr == addr && v.frees[0].err == hipSuccess, "plain block not hipFree'd");
    }
    check_all();
    return o;
  }

  // a free the allocator must refuse without touching the driver or its state
  void bad_free(uintptr_t addr) {
    DevMemStats a, b;
    gs_devmem_stats(&a);
    const size_t m = mark();
    const hipError_t e = gs_dev_free((void*)addr);
    const LogView v = since(m);
    CHECK(v.frees.empty(), "a bad free of %#zx reached hipFree", (size_t)addr);
    CHECK(e == hipErrorInvalidValue, "a bad free returned %d", (int)e);
    gs_devmem_stats(&b);
    CHECK(a.hip_allocs == b.hip_allocs && a.cache_hits == b.cache_hits && a.cached_bytes == b.cached_bytes &&
          a.mapped_bytes == b.mapped_bytes);
    check_all();
  }

  size_t trim(int device) {
    std::vector<size_t> predicted;
    for (const MSlab& s : slabs)
      if (s.all_free() && (device < 0 || s.dev == device)) predicted.push_back(s.size);
    std::sort(predicted.begin(), predicted.end());
    size_t sum = 0;
    for (size_t s : predicted) sum += s;
    const size_t m = mark();
    const size_t got = gs_devmem_trim(device);
    const LogView v = since(m);
    CHECK(got == sum, "trim returned %zu, model says %zu", got, sum);
    CHECK(v.mallocs == 0);
    apply_trims(v.frees, device, predicted);
    check_all();
    return got;
  }

  void set_device(int d) {
    CHECK(hipSetDevice(d) == hipSuccess);
    cur = d;
  }

  // gs_devmem_largest is honest: that many bytes can be had at once without a
  // hipFree, and without a hipMalloc if the figure was a cached extent
  void probe_largest() {
    const size_t L = gs_devmem_largest();
    CHECK(L == predict_largest(cur));
    if (!L) return;
    std::vector<size_t> whole, part;
    free_extents(cur, whole, part);
    const bool from_cache = enabled && best_fit(whole, part, L) == L;
    const size_t m = mark();
    const Outcome o = malloc(L);
    const LogView v = since(m);
    CHECK(o.err == hipSuccess, "gs_devmem_largest() = %zu cannot be had", L);
    CHECK(v.frees.empty(), "gs_devmem_largest() = %zu needed %zu hipFree(s)", L, v.frees.size());
    if (from_cache) CHECK(v.mallocs == 0 && o.cls == HIT);
    ++seen[from_cache ? "largest_cached" : "largest_new"];
    free(o.addr);
  }

  void check_all() {
    Fake& f = fk();
    DevMemStats st;
    gs_devmem_stats(&st);
    uint64_t mapped = 0, used = 0;
    for (const MSlab& s : slabs) {
      mapped += s.size;
      uintptr_t at = s.base;
      for (size_t i = 0; i < s.ext.size(); ++i) {
        CHECK(s.ext[i].addr == at && s.ext[i].size > 0);
        CHECK(i == 0 || s.ext[i].used || s.ext[i - 1].used);
        at += s.ext[i].size;
        if (s.ext[i].used) used += s.ext[i].size;
      }
      CHECK(at == s.base + s.size);
    }
    int hd = -1;
    CHECK(hipGetDevice(&hd) == hipSuccess && hd == cur, "the current device is %d, was %d", hd, cur);
    const size_t L = gs_devmem_largest(), PL = predict_largest(cur);
    CHECK(L == PL, "gs_devmem_largest() %zu, model %zu", L, PL);
    std::lock_guard<std::mutex> g(f.mu);
    CHECK(st.hip_allocs == f.n_malloc, "hip_allocs %" PRIu64 " vs %" PRIu64 " calls", st.hip_allocs, f.n_malloc);
    CHECK(st.mapped_bytes == mapped, "mapped_bytes %" PRIu64 " vs %" PRIu64, st.mapped_bytes, mapped);
    CHECK(st.cached_bytes == mapped - used, "cached_bytes %" PRIu64 " vs %" PRIu64, st.cached_bytes, mapped - used);
    // requests served without mapping memory (a hit after a hipMalloc failed for lack of room is one)
    CHECK(st.cache_hits == hits, "cache_hits %" PRIu64 " vs %" PRIu64, st.cache_hits, hits);
    CHECK(f.unknown_free == 0 && f.freed_under_block == 0);
    // the driver holds the model's slabs and the plain blocks, nothing else
    size_t plain = 0;
    for (const Block& b : blocks) plain += !b.cached;
    CHECK(f.live.size() == slabs.size() + plain, "%zu driver allocations, model %zu", f.live.size(), slabs.size() + plain);
    for (const MSlab& s : slabs) {
      auto it = f.live.find(s.base);
      CHECK(it != f.live.end() && it->second.size == s.size && it->second.dev == s.dev);
    }
    // every block inside one live allocation of its device, no two overlapping
    std::vector<std::pair<uintptr_t, size_t>> span;
    for (const Block& b : blocks) {
      const size_t n = b.cached ? round_up(b.bytes) : b.bytes;
      auto it = f.live.upper_bound(b.addr);
      CHECK(it != f.live.begin());
      --it;
      CHECK(b.addr + n <= it->first + it->second.size && it->second.dev == b.dev, "block outside a live allocation");
      span.push_back({b.addr, n});
    }
    std::sort(span.begin(), span.end());
    for (size_t i = 1; i < span.size(); ++i) CHECK(span[i - 1].first + span[i - 1].second <= span[i].first, "overlap");
  }

  // everything freed: one trim returns every mapped byte (coalescing is complete)
  void finish() {
    while (!blocks.empty()) free(blocks.back().addr);
    DevMemStats st;
    gs_devmem_stats(&st);
    const size_t got = trim(-1);
    CHECK(got == st.mapped_bytes, "trim(-1) %zu of %" PRIu64 " mapped", got, st.mapped_bytes);
    gs_devmem_stats(&st);
    CHECK(st.cached_bytes == 0 && st.mapped_bytes == 0 && slabs.empty());
    CHECK(fk().live.empty());
  }
  // the device as if other processes held the rest: `room` bytes free now
  void set_room(int d, size_t room) {
    Fake& f = fk();
    std::lock_guard<std::mutex> g(f.mu);
    f.capacity[d] = f.live_bytes[d] + room;
  }
};

std::string report(const Sim& s) {
  std::string r = "{";
  for (const auto& kv : s.seen) r += (r.size() > 1 ? ", \"" : "\"") + kv.first + "\": " + std::to_string(kv.second);
  return r + "}";
}
void ok(const std::string& extra = "{}") {
  printf("{\"scenario\": \"%s\", \"ok\": true, \"seen\": %s}\n", g_scenario.c_str(), extra.c_str());
}
std::vector<size_t> sizes(std::initializer_list<size_t> l) { return std::vector<size_t>(l); }

// ------------------------------------------------------- randomised sequences
void run_random(unsigned seed) {
  static const size_t kSizes[] = {1 * MiB, 63 * MiB, 64 * MiB, 64 * MiB + 1, 100 * MiB, GiB - 1, 3 * GiB, 9 * GiB, 40 * GiB};
  Sim s;
  std::mt19937_64 rng(seed * 0x9E3779B97F4A7C15ull + 1);
  auto pick = [&](uint64_t n) { return (size_t)(rng() % n); };
  // phases of growth and decline, so that the devices fill up and drain
  for (int op = 0; op < 2000; ++op) {
    const bool grow = (op / 250) % 2 == 0;
    const size_t r = pick(100);
    char ctx[96];
    if (r < (grow ? 58u : 34u)) {
      const size_t b = kSizes[pick(9)];
      snprintf(ctx, sizeof ctx, "seed %u op %d: malloc %zu on device %d", seed, op, b, s.cur);
      g_ctx = ctx;
      s.malloc(b);
    } else if (r < 88) {
      if (s.blocks.empty()) continue;
      const Block b = s.blocks[pick(s.blocks.size())];
      snprintf(ctx, sizeof ctx, "seed %u op %d: free %zu of device %d (current %d)", seed, op, b.bytes, b.dev, s.cur);
      g_ctx = ctx;
      s.free(b.addr);
    } else if (r < 94) {
      s.set_device((int)pick(kDevices));
    } else if (r < 96) {
      const int d = (int)pick(kDevices + 1) - 1;
      snprintf(ctx, sizeof ctx, "seed %u op %d: trim %d", seed, op, d);
      g_ctx = ctx;
      s.trim(d);
    } else {
      snprintf(ctx, sizeof ctx, "seed %u op %d: largest on device %d", seed, op, s.cur);
      g_ctx = ctx;
      s.probe_largest();
    }
  }
  g_ctx = "end";
  s.finish();
  ok(report(s));
}

// --------------------------------------------------------- directed scenarios
void double_free() {
  Sim s;
  // (a) the block stayed its own extent (here: a whole slab)
  g_ctx = "own extent";
  uintptr_t a = s.malloc(GiB).addr;
  s.free(a);
  s.bad_free(a);
  Outcome o = s.malloc(GiB);
  CHECK(o.cls == HIT && o.addr == a);
  s.finish();
  // (b) the block was merged into the free extent before it: its address is
  // now interior to a free extent
  g_ctx = "coalesced into predecessor";
  uintptr_t slab = s.malloc(256 * MiB).addr;
  s.free(slab);
  a = s.malloc(128 * MiB).addr;
  uintptr_t b = s.malloc(128 * MiB).addr;
  CHECK(a == slab && b == slab + 128 * MiB);
  s.free(a);
  s.free(b);
  s.bad_free(b);
  o = s.malloc(128 * MiB);
  CHECK(o.cls == HIT && o.ext_size == 256 * MiB);
  s.finish();
  // (c) addresses inside a live slab that start no extent: in a live block, and in a free tail
  g_ctx = "not an extent start";
  a = s.malloc(256 * MiB).addr;
  s.bad_free(a + 4096);
  s.bad_free(a + 128 * MiB);
  s.free(a);
  a = s.malloc(128 * MiB).addr;
  s.bad_free(a + 192 * MiB);
  s.bad_free(a + 128 * MiB);  // the free tail's own start
  o = s.malloc(128 * MiB);
  CHECK(o.cls == HIT && o.addr == a + 128 * MiB);
  s.finish();
  // plain blocks (below the threshold) and addresses the cache never saw still go to hipFree
  g_ctx = "plain block";
  a = s.malloc(GiB).addr;
  uintptr_t p = s.malloc(MiB).addr;
  CHECK(p > a + GiB);
  size_t m = Sim::mark();
  s.free(p);
  CHECK(Sim::since(m).frees.size() == 1);
  s.finish();
  ok(report(s));
}

void picky_best_fit() {
  Sim s;
  auto free_extent = [&](size_t bytes) {  // one fully free slab of that size
    const uintptr_t a = s.malloc(bytes).addr;
    s.free(a);
    return a;
  };
  g_ctx = "64 MiB against 8 GiB";
  free_extent(8 * GiB);
  Outcome o = s.malloc(64 * MiB);
  CHECK(o.cls == NEW_SLAB && o.trimmed.empty() && o.mallocs == 1);
  CHECK(s.trim(-1) == 8 * GiB);  // the big extent stayed whole
  s.finish();
  g_ctx = "3 GiB against 8 GiB";
  free_extent(8 * GiB);
  o = s.malloc(3 * GiB);
  CHECK(o.cls == HIT && o.ext_size == 8 * GiB && o.mallocs == 0);
  s.finish();
  g_ctx = "128 MiB against 1 GiB";
  free_extent(GiB);
  o = s.malloc(128 * MiB);
  CHECK(o.cls == HIT && o.ext_size == GiB);
  s.finish();
  g_ctx = "exactly 4x";
  free_extent(8 * GiB);
  o = s.malloc(2 * GiB);
  CHECK(o.cls == HIT && o.ext_size == 8 * GiB);
  s.finish();
  g_ctx = "one granule over 4x";
  free_extent(8 * GiB + kGran);
  o = s.malloc(2 * GiB);
  CHECK(o.cls == NEW_SLAB);
  s.finish();
  g_ctx = "exactly 1 GiB over";
  free_extent(GiB + 128 * MiB);
  o = s.malloc(128 * MiB);
  CHECK(o.cls == HIT && o.ext_size == GiB + 128 * MiB);
  s.finish();
  g_ctx = "one granule more than 1 GiB over";
  free_extent(GiB + 128 * MiB + kGran);
  o = s.malloc(128 * MiB);
  CHECK(o.cls == NEW_SLAB);
  s.finish();
  // the incident: a small buffer must not pin the big slab that a later big
  // request needs back from the cache
  g_ctx = "m8 incident";
  free_extent(8 * GiB);
  s.set_room(0, 8 * GiB + 128 * MiB);
  o = s.malloc(64 * MiB);
  CHECK(o.cls == NEW_SLAB && o.trimmed.empty());
  o = s.malloc(9 * GiB);  // room 8 GiB + 64 MiB: only with the 8 GiB slab back
  CHECK(o.cls == NEW_SLAB && o.trimmed == sizes({8 * GiB}), "the big request did not get the slab back");
  s.set_room(0, 64 * GiB);
  s.finish();
  ok(report(s));
}

void no_room() {
  Sim s;
  // a 6 GiB free extent beside a live block, and a device with nothing left
  g_ctx = "relaxed fit";
  uintptr_t a = s.malloc(8 * GiB).addr;
  s.free(a);
  a = s.malloc(2 * GiB).addr;
  s.set_room(0, 0);
  Outcome o = s.malloc(64 * MiB);
  CHECK(o.cls == HIT && o.relaxed && o.ext_size == 6 * GiB && o.mallocs == 1 && o.trimmed.empty());
  CHECK(o.addr == a + 2 * GiB);
  // nothing fits and nothing to trim: the error, and the books as they were
  g_ctx = "nothing to trim";
  DevMemStats b0, b1;
  gs_devmem_stats(&b0);
  o = s.malloc(7 * GiB);
  CHECK(o.cls == FAIL && o.mallocs == 1 && o.err == hipErrorOutOfMemory);
  gs_devmem_stats(&b1);
  CHECK(b1.hip_allocs == b0.hip_allocs + 1 && b1.cache_hits == b0.cache_hits && b1.cached_bytes == b0.cached_bytes &&
        b1.mapped_bytes == b0.mapped_bytes);
  s.set_room(0, 64 * GiB);
  s.finish();
  // the driver refuses although it reports the room (fragmentation): every
  // free slab goes back and the second try succeeds
  g_ctx = "trim all and retry";
  uintptr_t t1 = s.malloc(GiB).addr, t2 = s.malloc(2 * GiB).addr, live = s.malloc(GiB).addr;
  s.free(t1);
  s.free(t2);
  fk().fail_next = 1;
  o = s.malloc(3 * GiB);
  CHECK(o.cls == NEW_SLAB && o.mallocs == 2 && o.trimmed == sizes({GiB, 2 * GiB}));
  CHECK(s.slabs.size() == 2);  // the slab with the live block stayed
  (void)live;
  // ... and fails for good when the second try fails too
  g_ctx = "retry fails";
  s.free(o.addr);
  fk().fail_next = 2;
  o = s.malloc(4 * GiB);
  CHECK(o.cls == FAIL && o.mallocs == 2 && o.trimmed == sizes({3 * GiB}));
  // a device too small from the start
  g_ctx = "small device";
  s.set_device(1);
  s.set_room(1, 512 * MiB);
  o = s.malloc(GiB);
  CHECK(o.cls == FAIL && o.mallocs == 1);
  o = s.malloc(256 * MiB);  // fits, without the margin
  CHECK(o.cls == NEW_SLAB);
  s.set_device(0);
  s.finish();
  ok(report(s));
}

void trim_to_fit() {
  Sim s;
  auto three = [&] {
    uintptr_t a = s.malloc(GiB).addr, b = s.malloc(2 * GiB).addr, c = s.malloc(4 * GiB).addr;
    s.free(a);
    s.free(b);
    s.free(c);
  };
  g_ctx = "smallest single slab";
  three();
  s.set_room(0, 6 * GiB + kMargin - (GiB + 512 * MiB));  // short by 1.5 GiB
  size_t m = Sim::mark();
  Outcome o = s.malloc(6 * GiB);
  CHECK(o.cls == NEW_SLAB && o.trimmed == sizes({2 * GiB}) && o.mallocs == 1);
  CHECK(Sim::since(m).frees.size() == 1);
  s.set_room(0, 64 * GiB);
  s.finish();
  g_ctx = "largest first";
  three();
  s.set_room(0, 6 * GiB + kMargin - 5 * GiB);  // short by 5 GiB: no single slab covers it
  m = Sim::mark();
  o = s.malloc(6 * GiB);
  CHECK(o.cls == NEW_SLAB && o.trimmed == sizes({2 * GiB, 4 * GiB}));
  const auto fr = Sim::since(m).frees;
  CHECK(fr.size() == 2 && fr[0].size == 4 * GiB && fr[1].size == 2 * GiB);
  s.set_room(0, 64 * GiB);
  CHECK(s.trim(-1) == GiB);  // the third stayed cached
  s.finish();
  ok(report(s));
}

void margin() {
  Sim s;
  g_ctx = "exactly need + margin";
  uintptr_t t = s.malloc(64 * MiB).addr;
  s.free(t);
  s.set_room(0, GiB + kMargin);
  Outcome o = s.malloc(GiB);
  CHECK(o.cls == NEW_SLAB && o.trimmed.empty());
  s.free(o.addr);  // room is 8 GiB now: no trim
  CHECK(s.trim(-1) == GiB + 64 * MiB);
  g_ctx = "one granule short";
  t = s.malloc(64 * MiB).addr;
  s.free(t);
  s.set_room(0, GiB + kMargin - kGran);
  o = s.malloc(GiB);
  CHECK(o.cls == NEW_SLAB && o.trimmed == sizes({64 * MiB}));
  s.free(o.addr);
  s.set_room(0, 64 * GiB);
  s.finish();
  g_ctx = "headroom after a free";
  uintptr_t a = s.malloc(GiB).addr, b = s.malloc(3 * GiB).addr, c = s.malloc(GiB).addr;
  s.free(a);
  s.free(b);
  s.set_room(0, 7 * GiB + 512 * MiB);
  o = s.free(c);  // short by 512 MiB: one of the 1 GiB slabs, not the 3 GiB one
  CHECK(o.trimmed == sizes({GiB}));
  s.set_room(0, 2 * GiB);
  uintptr_t d = s.malloc(64 * MiB).addr;  // best fit: from the 1 GiB slab
  CHECK(s.slabs.size() == 2);
  o = s.free(d);  // short by 6 GiB - 64 MiB: the largest first, then the other: both
  CHECK(o.trimmed == sizes({GiB, 3 * GiB}));
  g_ctx = "largest";
  CHECK(gs_devmem_largest() == 0);  // 6 GiB free, nothing cached
  s.set_room(0, kMargin + 5 * MiB);
  CHECK(gs_devmem_largest() == 5 * MiB);
  s.set_room(0, 64 * GiB);
  a = s.malloc(GiB).addr;
  s.free(a);
  s.set_room(0, kMargin + 512 * MiB);
  CHECK(gs_devmem_largest() == GiB);
  s.set_room(0, kMargin + 2 * GiB + MiB);
  CHECK(gs_devmem_largest() == 2 * GiB);  // a cached-size request is rounded up to 2 MiB
  s.probe_largest();
  s.set_room(0, 64 * GiB);
  s.finish();
  ok(report(s));
}

void bypass_small() {
  Sim s;
  CHECK(s.enabled);
  DevMemStats a, b;
  gs_devmem_stats(&a);
  const size_t m = Sim::mark();
  for (size_t bytes : {(size_t)1, 4096 * (size_t)1, MiB, 63 * MiB, kMin - 1}) {
    Outcome o = s.malloc(bytes);
    CHECK(o.cls == PLAIN);
    s.free(o.addr);
  }
  const auto v = Sim::since(m);
  CHECK(v.mallocs == 5 && v.frees.size() == 5 && v.syncs == 0);
  gs_devmem_stats(&b);
  CHECK(b.hip_allocs == a.hip_allocs + 5 && b.cache_hits == 0 && b.cached_bytes == 0 && b.mapped_bytes == 0);
  s.finish();
  ok(report(s));
}

void bypass_off() {  // run with GS_DEVMEM_CACHE=0
  Sim s;
  CHECK(!s.enabled, "this scenario needs GS_DEVMEM_CACHE=0");
  const size_t m = Sim::mark();
  std::vector<uintptr_t> held;
  for (size_t bytes : {MiB, kMin, 3 * GiB, 40 * GiB}) {
    Outcome o = s.malloc(bytes);
    CHECK(o.cls == PLAIN);
    held.push_back(o.addr);
  }
  for (uintptr_t a : held) s.free(a);
  const auto v = Sim::since(m);
  CHECK(v.mallocs == 4 && v.frees.size() == 4);
  for (size_t i = 0; i < 4; ++i) CHECK(v.frees[i].addr == held[i]);
  DevMemStats b;
  gs_devmem_stats(&b);
  CHECK(b.hip_allocs == 4 && b.cache_hits == 0 && b.cached_bytes == 0 && b.mapped_bytes == 0);
  // a second free is the driver's business here, as with hipFree itself
  CHECK(gs_dev_free((void*)held[1]) == hipErrorInvalidValue);
  CHECK(fk().unknown_free == 1);
  fk().unknown_free = 0;
  s.set_room(0, kMargin + 3 * GiB + 1);
  CHECK(gs_devmem_largest() == 3 * GiB + 1);
  s.set_room(0, kMargin);
  CHECK(gs_devmem_largest() == 0);
  CHECK(gs_devmem_trim(-1) == 0);
  s.set_room(0, 64 * GiB);
  s.finish();
  ok(report(s));
}

void devices() {
  Sim s;
  s.set_device(1);
  uintptr_t a = s.malloc(GiB).addr;
  s.set_device(0);
  size_t m = Sim::mark();
  s.free(a);  // checks the sync on device 1 and that device 0 is current again
  bool went = false, back = false;
  {
    std::lock_guard<std::mutex> g(fk().mu);
    for (size_t i = m; i < fk().log.size(); ++i)
      if (fk().log[i].kind == 'S') (fk().log[i].dev == 1 ? went : back) = true;
  }
  CHECK(went && back);
  Outcome o = s.malloc(GiB);  // device 0 has nothing cached
  CHECK(o.cls == NEW_SLAB && o.addr != a);
  s.set_room(0, 0);
  Outcome f = s.malloc(GiB);  // not even with no room is device 1's extent taken
  CHECK(f.cls == FAIL);
  s.set_room(0, 64 * GiB);
  s.set_device(1);
  Outcome h = s.malloc(GiB);
  CHECK(h.cls == HIT && h.addr == a);
  s.free(h.addr);
  s.set_device(2);
  s.free(o.addr);  // device 0's block, freed from device 2
  CHECK(s.trim(1) == GiB);
  CHECK(s.slabs.size() == 1 && s.slabs[0].dev == 0);
  CHECK(s.trim(2) == 0);
  CHECK(s.trim(0) == GiB);
  s.set_device(0);
  s.finish();
  ok(report(s));
}

void split_coalesce() {
  Sim s;
  const size_t q = 128 * MiB;
  uintptr_t base = s.malloc(4 * q).addr;
  s.free(base);
  s.set_room(0, kMargin);  // gs_devmem_largest() is the largest free extent from here on
  uintptr_t a = s.malloc(q).addr, b = s.malloc(q).addr, c = s.malloc(q).addr;
  Outcome last = s.malloc(q);  // takes the rest whole: no empty extent is split off
  uintptr_t d = last.addr;
  CHECK(last.cls == HIT && last.ext_size == q);
  CHECK(a == base && b == base + q && c == base + 2 * q && d == base + 3 * q);
  CHECK(gs_devmem_largest() == 0);
  g_ctx = "neither";
  s.free(b);
  CHECK(gs_devmem_largest() == q);
  g_ctx = "previous only";
  s.free(c);
  CHECK(gs_devmem_largest() == 2 * q);
  g_ctx = "next only";
  s.free(a);
  CHECK(gs_devmem_largest() == 3 * q);
  a = s.malloc(q).addr;
  b = s.malloc(q).addr;
  CHECK(a == base && b == base + q && gs_devmem_largest() == q);
  s.free(d);  // previous only, at the slab's end
  CHECK(gs_devmem_largest() == 2 * q);
  s.free(a);  // neither, at the slab's start
  CHECK(gs_devmem_largest() == 2 * q);
  g_ctx = "both";
  s.free(b);
  CHECK(gs_devmem_largest() == 4 * q);
  // a request rounded up to the granule that leaves no rest
  Outcome o = s.malloc(4 * q - 1);
  CHECK(o.cls == HIT && o.addr == base && gs_devmem_largest() == 0);
  s.free(o.addr);
  s.set_room(0, 64 * GiB);
  s.finish();
  // two slabs back to back are two extents
  g_ctx = "adjacent slabs";
  fk().contiguous = true;
  uintptr_t x = s.malloc(q).addr, y = s.malloc(q).addr;
  fk().contiguous = false;
  CHECK(y == x + q);
  s.set_room(0, kMargin);
  s.free(x);
  s.free(y);
  CHECK(gs_devmem_largest() == q);
  o = s.malloc(2 * q);
  CHECK(o.cls == NEW_SLAB && o.trimmed == sizes({q, q}) && o.mallocs == 1);  // short of room by both
  s.set_room(0, 64 * GiB);
  s.finish();
  ok(report(s));
}

// the poison switch on: every kind of successful request is filled (checked
// in Sim::malloc), and a failed fill hands out nothing
void poison_on() {  // run with GS_DEVMEM_POISON set
  Sim s;
  CHECK(s.poison, "this scenario needs GS_DEVMEM_POISON");
  g_ctx = "plain";
  Outcome o = s.malloc(MiB);
  CHECK(o.cls == PLAIN);
  o = s.malloc(kMin - 1);
  CHECK(o.cls == PLAIN);
  g_ctx = "new slab";
  o = s.malloc(GiB + 1);  // rounded up: the fill covers the whole extent
  CHECK(o.cls == NEW_SLAB);
  const uintptr_t slab = o.addr;
  s.free(slab);
  g_ctx = "hit after a split";
  o = s.malloc(256 * MiB);
  CHECK(o.cls == HIT && o.ext_size == GiB + kGran && o.addr == slab);
  o = s.malloc(128 * MiB + 5);
  CHECK(o.cls == HIT && o.addr == slab + 256 * MiB);
  o = s.malloc(640 * MiB);  // the rest, whole
  CHECK(o.cls == HIT && o.ext_size == 640 * MiB);
  g_ctx = "fallback after a failed hipMalloc";
  uintptr_t t = s.malloc(8 * GiB).addr;
  s.free(t);
  o = s.malloc(2 * GiB);
  CHECK(o.cls == HIT && o.addr == t);
  s.set_room(0, 0);
  o = s.malloc(64 * MiB);  // hipMalloc fails for lack of room: the relaxed fit
  CHECK(o.cls == HIT && o.relaxed && o.mallocs == 1 && o.addr == t + 2 * GiB);
  s.set_room(0, 64 * GiB);
  while (!s.blocks.empty()) s.free(s.blocks.back().addr);
  fk().fail_next = 1;
  o = s.malloc(9 * GiB);  // the driver refuses once: every free slab back, then a new slab
  CHECK(o.cls == NEW_SLAB && o.mallocs == 2 && o.trimmed == sizes({GiB + kGran, 8 * GiB}));
  s.free(o.addr);
  g_ctx = "failed fill: plain";
  o = s.malloc_fill_fails(MiB);
  CHECK(o.cls == PLAIN);
  s.check_all();
  g_ctx = "failed fill: hit";
  o = s.malloc_fill_fails(3 * GiB);
  CHECK(o.cls == HIT && o.ext_size == 9 * GiB);
  s.check_all();
  o = s.malloc(9 * GiB);  // the extent was put back whole
  CHECK(o.cls == HIT && o.ext_size == 9 * GiB);
  s.free(o.addr);
  g_ctx = "failed fill: new slab";
  o = s.malloc_fill_fails(64 * MiB);  // 9 GiB free is far too big for it: a slab of its own
  CHECK(o.cls == NEW_SLAB);
  s.check_all();
  o = s.malloc(64 * MiB);  // which now serves the same request
  CHECK(o.cls == HIT && o.ext_size == 64 * MiB);
  s.finish();
  ok(report(s));
}

// the switch off (unset, or a value out of range): the directed requests of
// every kind log no fill; Sim::malloc checks the same in every other scenario
void poison_off() {
  Sim s;
  CHECK(!s.poison, "this scenario needs GS_DEVMEM_POISON unset or out of range");
  const size_t m = Sim::mark();
  Outcome o = s.malloc(MiB);
  CHECK(o.cls == PLAIN);
  o = s.malloc(8 * GiB);
  CHECK(o.cls == NEW_SLAB);
  s.free(o.addr);
  o = s.malloc(2 * GiB);
  CHECK(o.cls == HIT);
  s.set_room(0, 0);
  o = s.malloc(64 * MiB);
  CHECK(o.cls == HIT && o.relaxed);
  s.set_room(0, 64 * GiB);
  s.finish();
  const auto v = Sim::since(m);
  CHECK(v.fills.empty(), "%zu fill(s) with the switch off", v.fills.size());
  ok(report(s));
}

// ---------------------------------------------------------------------- threads
void threads() {
  static const size_t kSizes[] = {1 * MiB, 64 * MiB, 64 * MiB + 1, 100 * MiB, 512 * MiB, GiB - 1, 3 * GiB};
  constexpr int kThreads = 8, kOps = 500, kHold = 8;
  std::atomic<bool> stop{false};
  std::atomic<int> bad{0};
  std::vector<std::vector<Block>> held(kThreads);
  auto worker = [&](int id) {
    (void)hipSetDevice(id % 2);
    std::mt19937_64 rng(1000 + id);
    std::vector<Block>& mine = held[id];
    Fake& f = fk();
    for (int op = 0; op < kOps; ++op) {
      if (mine.size() < kHold && (mine.empty() || rng() % 100 < 55)) {
        const size_t bytes = kSizes[rng() % 7];
        void* p = nullptr;
        if (gs_dev_malloc(&p, bytes) != hipSuccess) {
          ++bad;
          continue;
        }
        const uintptr_t a = (uintptr_t)p;
        const size_t n = bytes >= kMin ? round_up(bytes) : bytes;
        std::lock_guard<std::mutex> g(f.mu);
        auto it = f.live.upper_bound(a);  // a block sits in a live allocation of the thread's device
        if (it == f.live.begin() || (--it, a + n > it->first + it->second.size) || it->second.dev != id % 2) ++bad;
        auto nb = f.blocks.lower_bound(a);  // and overlaps no other thread's block
        if (nb != f.blocks.end() && nb->first < a + n) ++bad;
        if (nb != f.blocks.begin() && (--nb, nb->first + nb->second > a)) ++bad;
        f.blocks[a] = n;
        mine.push_back({a, bytes, id % 2, bytes >= kMin});
      } else {
        const size_t i = rng() % mine.size();
        {
          std::lock_guard<std::mutex> g(f.mu);
          f.blocks.erase(mine[i].addr);
        }
        if (gs_dev_free((void*)mine[i].addr) != hipSuccess) ++bad;
        mine.erase(mine.begin() + i);
      }
    }
  };
  std::thread trimmer([&] {
    DevMemStats st;
    while (!stop) {
      gs_devmem_trim(-1);
      gs_devmem_stats(&st);
      if (st.cached_bytes > st.mapped_bytes) ++bad;
      (void)gs_devmem_largest();
      std::this_thread::yield();
    }
  });
  std::vector<std::thread> th;
  for (int i = 0; i < kThreads; ++i) th.emplace_back(worker, i);
  for (auto& t : th) t.join();
  stop = true;
  trimmer.join();
  CHECK(bad == 0, "%d violations while the threads ran", bad.load());
  Fake& f = fk();
  DevMemStats st;
  gs_devmem_stats(&st);
  uint64_t mapped = 0, used = 0;
  for (const auto& kv : f.live)
    if (kv.second.size >= kMin) mapped += kv.second.size;
  std::vector<std::pair<uintptr_t, size_t>> span;
  for (const auto& mine : held)
    for (const Block& b : mine) {
      const size_t n = b.cached ? round_up(b.bytes) : b.bytes;
      if (b.cached) used += n;
      auto it = f.live.upper_bound(b.addr);
      CHECK(it != f.live.begin());
      --it;
      CHECK(b.addr + n <= it->first + it->second.size && it->second.dev == b.dev);
      span.push_back({b.addr, n});
    }
  std::sort(span.begin(), span.end());
  for (size_t i = 1; i < span.size(); ++i) CHECK(span[i - 1].first + span[i - 1].second <= span[i].first, "overlap");
  CHECK(st.hip_allocs == f.n_malloc);
  CHECK(st.mapped_bytes == mapped, "mapped_bytes %" PRIu64 " vs %" PRIu64, st.mapped_bytes, mapped);
  CHECK(st.cached_bytes == mapped - used);
  CHECK(f.unknown_free == 0 && f.freed_under_block == 0);
  for (auto& mine : held)
    for (const Block& b : mine) {
      f.blocks.erase(b.addr);
      CHECK(gs_dev_free((void*)b.addr) == hipSuccess);
    }
  gs_devmem_stats(&st);
  CHECK(gs_devmem_trim(-1) == st.mapped_bytes);
  gs_devmem_stats(&st);
  CHECK(st.cached_bytes == 0 && st.mapped_bytes == 0 && f.live.empty());
  CHECK(f.unknown_free == 0 && f.freed_under_block == 0);
  ok("{\"hip_allocs\": " + std::to_string(st.hip_allocs) + ", \"cache_hits\": " + std::to_string(st.cache_hits) + "}");
}

// -------------------------------------------------------------------- planner
typedef unsigned long long ull;

// the passes, restated: a pass takes bins while its records fit `cap`
std::vector<uint32_t> plain_cuts(const std::vector<ull>& need, ull cap) {
  std::vector<uint32_t> cut{0};
  size_t c = 0;
  while (c < need.size()) {
    ull sum = need[c++];
    while (c < need.size() && sum + need[c] <= cap) sum += need[c++];
    cut.push_back((uint32_t)c);
  }
  return cut;
}
// the block sized as the largest coarse copy plus the largest fine copy, one
// split for all passes (what the build did before gs_rev_plan.h)
ull split_once_size(const std::vector<ull>& h, const std::vector<ull>& need, const std::vector<uint32_t>& cut) {
  ull rm = 1, fm = 1;
  for (size_t p = 0; p + 1 < cut.size(); ++p) {
    ull r = 0, f = 0;
    for (uint32_t c = cut[p]; c < cut[p + 1]; ++c) r += h[c], f += need[c] - h[c];
    rm = std::max(rm, r);
    fm = std::max(fm, f);
  }
  return rm + fm;
}

void check_plan(const std::vector<ull>& h, const std::vector<ull>& need, ull cap, ull forced, uint64_t* same_as_before) {
  const size_t nbins = h.size();
  const gs::RevPlan pl = gs::pp_rev_plan(h.data(), need.data(), nbins, cap, forced);
  const ull biggest = *std::max_element(need.begin(), need.end());
  if (!forced && biggest > cap) {
    CHECK(!pl.ok, "a plan although a bin does not fit");
    return;
  }
  CHECK(pl.ok, "no plan although every bin fits");
  const size_t P = pl.cut.size() - 1;
  CHECK(pl.cut.front() == 0 && pl.cut.back() == nbins && pl.rec.size() == P);
  for (size_t p = 0; p < P; ++p) {
    CHECK(pl.cut[p] < pl.cut[p + 1], "cuts not increasing");  // so every bin is in exactly one pass
    ull r = 0, sum = 0;
    for (uint32_t c = pl.cut[p]; c < pl.cut[p + 1]; ++c) r += h[c], sum += need[c];
    CHECK(pl.rec[p] == r);
    CHECK(sum <= pl.tmp_records, "pass %zu: %llu records in a block of %llu", p, sum, (ull)pl.tmp_records);
    if (!forced && p + 1 < P) CHECK(sum + need[pl.cut[p + 1]] > cap, "pass %zu could have taken the next bin", p);
  }
  if (forced) {
    const size_t per = (nbins + forced - 1) / forced;
    CHECK(P == (nbins + per - 1) / per);
    for (size_t p = 0; p < P; ++p) CHECK(pl.cut[p] == p * per);
    return;
  }
  CHECK(pl.tmp_records <= std::max<ull>(cap, 1), "block of %llu records, cap %llu", (ull)pl.tmp_records, cap);
  const std::vector<uint32_t> ref = plain_cuts(need, cap);
  if (split_once_size(h, need, ref) <= cap) {  // the earlier layout fitted as well: the same passes
    CHECK(pl.cut == ref);
    ++*same_as_before;
  }
  CHECK(pl.cut.size() == ref.size(), "%zu passes, %zu expected", P, ref.size() - 1);
}

void planner() {
  uint64_t same = 0, plans = 0;
  for (unsigned seed = 1; seed <= 40; ++seed) {
    std::mt19937_64 rng(seed);
    const size_t nbins = seed == 1 ? 1 : seed == 2 ? 512 : 1 + rng() % 512;
    std::vector<ull> h(nbins), need(nbins);
    const int shape = seed % 4;  // even, coarse-heavy, fine-heavy, mixed per bin
    for (size_t c = 0; c < nbins; ++c) {
      const ull a = rng() % 1000000, b = rng() % 1000000;
      const int sh = shape == 3 ? (int)(rng() % 3) : shape;
      h[c] = sh == 2 ? a / 64 : a;
      need[c] = h[c] + (sh == 1 ? b / 64 : b) + 1024;
    }
    ull total = 0, biggest = 0;
    for (ull v : need) total += v, biggest = std::max(biggest, v);
    char ctx[64];
    for (ull cap : {biggest, biggest + 1, biggest * 2, biggest * 7 + 3, total / 3 + biggest, total - 1, total, total * 2,
                    biggest - 1, (ull)0}) {
      snprintf(ctx, sizeof ctx, "planner seed %u cap %llu", seed, cap);
      g_ctx = ctx;
      check_plan(h, need, cap, 0, &same);
      ++plans;
    }
    for (ull forced : {(ull)1, (ull)2, (ull)3, (ull)7, (ull)nbins, (ull)nbins + 5}) {
      snprintf(ctx, sizeof ctx, "planner seed %u forced %llu", seed, forced);
      g_ctx = ctx;
      check_plan(h, need, 0, forced, &same);
    }
  }
  // the adversarial pair: pass 0 has the largest coarse copy, pass 1 the largest fine copy
  g_ctx = "adversarial";
  {
    const std::vector<ull> h{90, 10}, need{100, 100};
    const ull cap = 100;
    CHECK(split_once_size(h, need, plain_cuts(need, cap)) == 180);  // the earlier block: over the cap
    const gs::RevPlan pl = gs::pp_rev_plan(h.data(), need.data(), 2, cap, 0);
    CHECK(pl.ok && pl.cut == std::vector<uint32_t>({0, 1, 2}));
    CHECK(pl.tmp_records <= cap, "block of %llu records for a cap of %llu", (ull)pl.tmp_records, cap);
    check_plan(h, need, cap, 0, &same);
    // the same with many bins per pass
    std::vector<ull> h2, n2;
    for (int i = 0; i < 8; ++i) h2.push_back(1000), n2.push_back(1100);
    for (int i = 0; i < 8; ++i) h2.push_back(100), n2.push_back(1100);
    CHECK(split_once_size(h2, n2, plain_cuts(n2, 8800)) > 8800);
    check_plan(h2, n2, 8800, 0, &same);
  }
  // N = 1e7 as the GPU test builds it (three coarse bins of 2^22 nodes): one pass by default, three when forced
  g_ctx = "n = 1e7";
  {
    const ull n = 10000000, nbins = (n + (1ull << 22) - 1) >> 22, nbf = (n + 16383) >> 14;
    std::vector<ull> h(nbins), need(nbins);
    for (ull c = 0; c < nbins; ++c) {
      const ull nodes_c = std::min<ull>(1ull << 22, n - (c << 22));
      h[c] = nodes_c * 11;
      need[c] = h[c];
      for (ull dd = 0; dd < std::min<ull>(256, nbf - c * 256); ++dd) {
        const ull nodes_b = std::min<ull>(16384, n - (c * 256 + dd) * 16384);
        const ull share = (ull)((double)h[c] * nodes_b / nodes_c);
        need[c] += share + share / 8 + 1024;
      }
    }
    CHECK(nbins == 3);
    const ull cap = (200ull << 30) / 8;
    CHECK(gs::pp_rev_plan(h.data(), need.data(), nbins, cap, 0).cut.size() == 2);
    CHECK(gs::pp_rev_plan(h.data(), need.data(), nbins, 0, 1).cut.size() == 2);
    CHECK(gs::pp_rev_plan(h.data(), need.data(), nbins, cap, 3).cut == std::vector<uint32_t>({0, 1, 2, 3}));
    check_plan(h, need, cap, 0, &same);
  }
  CHECK(same > 100, "only %" PRIu64 " plans compared with the earlier layout", same);
  ok("{\"plans\": " + std::to_string(plans) + ", \"same_as_before\": " + std::to_string(same) + "}");
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s <scenario>\n", argv[0]);
    return 2;
  }
  g_scenario = argv[1];
  const std::string s = argv[1];
  if (s.rfind("random:", 0) == 0)
    run_random((unsigned)atoi(s.c_str() + 7));
  else if (s == "double_free")
    double_free();
  else if (s == "picky_best_fit")
    picky_best_fit();
  else if (s == "no_room")
    no_room();
  else if (s == "trim_to_fit")
    trim_to_fit();
  else if (s == "margin")
    margin();
  else if (s == "bypass_small")
    bypass_small();
  else if (s == "bypass_off")
    bypass_off();
  else if (s == "devices")
    devices();
  else if (s == "split_coalesce")
    split_coalesce();
  else if (s == "poison")
    poison_on();
  else if (s == "poison_off")
    poison_off();
  else if (s == "threads")
    threads();
  else if (s == "planner")
    planner();
  else {
    fprintf(stderr, "unknown scenario %s\n", argv[1]);
    return 2;
  }
  return 0;
}
