// undba_san.cpp -- the host phases of csrc/brotli_undba.h (on undbp's walk and items, csrc/brotli_undbp.h) under AddressSanitizer and UBSan, as
// a program of its own:
//   g++ -std=c++17 -fsanitize=address,undefined -I include -I rust-brotli-decompressor_amd/csrc tests/tools/undba_san.cpp
// The two walks, the items' delta sums, the carries, the items' tests and sums, their carries, the offsets, and the phases A, B and C of the
// prefix copies, with items of 32, 64 and 96 deltas, forwards or backwards where the order is free, and with running strings of 8, 24 and
// 4096 bytes -- so that the walk back of phase A and the far bytes of phase B are taken for strings of a few dozen bytes --, against the
// strings the pages were made of: the examples of include/brotli/batch.h, and a seeded table of page bodies written by an encoder of its own --
// sorted strings behind stems of 0 .. 60 bytes, repeats and empty ones, one element that breaks one of the three rules, bodies cut short,
// capacities of m - 1, m and m + 5, data capacities that cut, both offset widths and ENDS_ONLY, seeded skews.  Every source lies in a heap
// block of EXACTLY the sixteen-byte words its span touches, and so do the offsets and the data that a segment delivers: a load or a store one
// word too far would be reported; the destinations' bytes beside what is delivered must keep their pattern.  Exits 0 when everything agreed.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "brotli_device_abi.h"
#include "brotli_undba.h"
#include "san_block.h"

static uint32_t g_seed = 8191u;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

typedef SanBlock Block;
typedef std::vector<uint8_t> Bytes;
typedef std::vector<std::string> Strings;

// ---- an encoder of its own: blocks of 128 values in 4 miniblocks ----
static void put_varint(Bytes* out, uint64_t v) { do { out->push_back((uint8_t)((v & 0x7Fu) | (v > 0x7Fu ? 0x80u : 0u))); v >>= 7; } while (v != 0u); }
static uint64_t zigzag(int64_t v) { return ((uint64_t)v << 1) ^ (uint64_t)(v >> 63); }
static void put_dbp(Bytes* out, const std::vector<int64_t>& vals) {
  put_varint(out, 128u); put_varint(out, 4u); put_varint(out, vals.size()); put_varint(out, vals.empty() ? 0u : zigzag(vals[0]));
  for (size_t at = 1; at < vals.size(); at += 128u) {
    const size_t n = std::min<size_t>(128u, vals.size() - at);
    int64_t md = INT64_MAX;
    for (size_t x = 0; x < n; x++) md = std::min(md, vals[at + x] - vals[at + x - 1u]);
    put_varint(out, zigzag(md));
    uint8_t widths[4] = {0, 0, 0, 0};
    for (size_t x = 0; x < n; x++) {
      const uint64_t f = (uint64_t)(vals[at + x] - vals[at + x - 1u] - md);
      uint8_t k = 0;
      while (k < 64u && (f >> k) != 0u) k++;
      widths[x / 32u] = std::max(widths[x / 32u], k);
    }
    out->insert(out->end(), widths, widths + 4);
    for (size_t mb = 0; mb * 32u < n; mb++) {
      const uint32_t k = widths[mb];
      Bytes packed(4u * k, 0);
      for (size_t x = mb * 32u; x < std::min(n, mb * 32u + 32u); x++) {
        const uint64_t f = (uint64_t)(vals[at + x] - vals[at + x - 1u] - md);
        for (uint32_t bit = 0; bit < k; bit++)
          if ((f >> bit) & 1u) packed[((x % 32u) * k + bit) / 8u] |= (uint8_t)(1u << (((x % 32u) * k + bit) % 8u));
      }
      out->insert(out->end(), packed.begin(), packed.end());
    }
  }
}
static size_t common(const std::string& a, const std::string& b) { size_t n = 0; while (n < a.size() && n < b.size() && a[n] == b[n]) n++; return n; }

struct Page { Bytes body; Strings want; std::vector<int64_t> prefixes; uint64_t first_bad; uint32_t kind; };   // want: the elements in front of first_bad
// the page of `strings`; bad_at < size: that element breaks `kind`
static Page make_page(const Strings& strings, size_t bad_at, uint32_t kind) {
  Page pg;
  std::vector<int64_t> p, s;
  Bytes tail;
  for (size_t i = 0; i < strings.size(); i++) {
    const size_t c = i ? std::min(common(strings[i - 1u], strings[i]), (size_t)(rnd() % 4u ? ~(size_t)0 : rnd() % 8u)) : 0u;   // (any shorter prefix is legal)
    p.push_back((int64_t)c); s.push_back((int64_t)(strings[i].size() - c));
    tail.insert(tail.end(), strings[i].begin() + (long)c, strings[i].end());
  }
  pg.first_bad = ~(uint64_t)0; pg.kind = BROTLI_AMD_UNDBA_BAD_NONE;
  if (bad_at < strings.size()) {
    if (kind == BROTLI_AMD_UNDBA_BAD_PREFIX_NEGATIVE) p[bad_at] = -1 - (int64_t)(rnd() % 1000u);
    else if (kind == BROTLI_AMD_UNDBA_BAD_SUFFIX_NEGATIVE) s[bad_at] = ((int64_t)7 << 32) + (int64_t)0x80000000u + (int64_t)(rnd() % 1000u);
    else p[bad_at] = (int64_t)(bad_at ? strings[bad_at - 1u].size() : 0u) + 1 + ((int64_t)5 << 32);
    pg.first_bad = bad_at; pg.kind = kind;
  }
  put_dbp(&pg.body, p); put_dbp(&pg.body, s);
  pg.prefixes = p;
  pg.body.insert(pg.body.end(), tail.begin(), tail.end());
  pg.want.assign(strings.begin(), strings.begin() + (long)std::min(bad_at, strings.size()));
  return pg;
}
static Strings make_strings(size_t n) {
  Strings out;
  const std::string stem(rnd() % 61u, (char)('a' + rnd() % 3u));
  for (size_t i = 0; i < n; i++) {
    std::string t = rnd() % 7u ? stem : std::string();
    for (uint32_t x = rnd() % 6u; x != 0u; x--) t.push_back((char)('a' + rnd() % 3u));
    out.push_back(t);
  }
  std::sort(out.begin(), out.end());
  return out;
}

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { std::printf(__VA_ARGS__); std::printf("\n"); if (++failures > 10) std::exit(1); } } while (0)

// One segment through every phase.  cut: bytes taken off the body's end (suffix bytes that then read as 0).
static void run(const Page& pg, size_t cut, uint64_t cap, uint64_t data_cap, uint32_t flags, uint32_t item, bool backwards, uint32_t string_cap, uint32_t carry_cap, const char* what) {
  const size_t len = pg.body.size() - cut;
  Block src(len, rnd() % 16u);
  for (size_t i = 0; i < src.span; i++) src.base[i] = (uint8_t)rnd();
  std::copy(pg.body.begin(), pg.body.begin() + (long)len, src.at());
  BrotliAmdUndbaSeg sg = {src.at(), nullptr, len, cap, 0u, flags, 0u, nullptr, data_cap, 1000u};
  uint64_t first_p = 0, first_s = 0;
  const uint64_t items = brotli_amd_undbp_items(cap, item);
  std::vector<BrotliAmdUndbpCheckpoint> cp_p(items, BrotliAmdUndbpCheckpoint{BROTLI_AMD_UNDBP_NONE, BROTLI_AMD_UNDBP_NONE}), cp_s(cp_p);
  BrotliAmdUndbaResult res = brotli_amd_undba_host_walk(sg, item, cp_p.data(), cp_s.data(), &first_p, &first_s);
  const uint64_t delivered = brotli_amd_undba_m(res.count_p, res.count_s, cap);
  Bytes want;
  std::vector<uint64_t> ends;
  for (uint64_t e = 0; e < delivered; e++) {
    if (e < pg.want.size()) want.insert(want.end(), pg.want[e].begin(), pg.want[e].end());
    ends.push_back(1000u + want.size());
  }
  // (cut suffix bytes read as 0: the strings' tails are the last bytes of the data where no element is bad)
  const uint32_t ow = brotli_amd_undlba_offset_width(flags);
  const bool ends_only = (flags & BROTLI_AMD_UNDBA_ENDS_ONLY) != 0u;
  Block offsets((delivered + (ends_only ? 0u : 1u)) * ow, rnd() % 16u);
  const uint64_t keep = std::min<uint64_t>(want.size(), data_cap);
  Block data(keep, rnd() % 16u);
  offsets.fill_pattern(); data.fill_pattern();
  sg.offsets = offsets.at(); sg.data = data.at();
  std::vector<uint64_t> order(items);
  for (uint64_t j = 0; j < items; j++) order[j] = backwards ? items - 1u - j : j;
  std::vector<BrotliAmdUndeltaTile> tp(items), ts(items), tl(items), tx(items);
  for (uint64_t j : order) brotli_amd_undba_host_sum(sg, res, cp_p[j], cp_s[j], first_p, first_s, j, item, &tp[j], &ts[j]);
  auto carries_of = [](const std::vector<BrotliAmdUndeltaTile>& t) {
    std::vector<uint64_t> c(t.size());
    BrotliAmdUndeltaPair out = {0u, 0u};
    for (size_t x = 0; x < t.size(); x++) { c[x] = brotli_amd_undelta_carry_in(out.sum, t[x]); out = brotli_amd_undelta_combine(out, brotli_amd_undelta_tile_pair(t[x])); }
    return c;
  };
  const std::vector<uint64_t> c_p = carries_of(tp), c_s = carries_of(ts);
  auto item_of = [&](uint64_t j) { return brotli_amd_undba_host_item(sg, res, cp_p[j], cp_s[j], first_p, first_s, j, item, c_p[j], c_s[j]); };
  for (uint64_t j : order) brotli_amd_undba_host_lengths(item_of(j), j, &res, &tl[j], &tx[j]);
  const std::vector<uint64_t> c_l = carries_of(tl), c_x = carries_of(tx);
  auto sums_in = [&](uint64_t j, uint64_t lo, uint64_t* bytes_in, uint64_t* suffix_in) {
    const uint64_t jb = lo > res.first_bad ? brotli_amd_undba_item_of(res.first_bad, item) : j;
    *bytes_in = brotli_amd_undba_sum_in(res.first_bad, lo, c_l[j], c_l[jb], tl[jb].sum);
    *suffix_in = brotli_amd_undba_sum_in(res.first_bad, lo, c_x[j], c_x[jb], tx[jb].sum);
  };
  uint64_t bytes_in, suffix_in;
  for (uint64_t j : order) {
    const BrotliAmdUndbaHostItem it = item_of(j);
    sums_in(j, it.lo, &bytes_in, &suffix_in);
    brotli_amd_undba_host_expand(sg, &res, it, j, item, bytes_in, suffix_in);
  }
  CHECK(res.first_bad == (pg.first_bad < delivered ? pg.first_bad : ~(uint64_t)0) && res.bad_kind == (pg.first_bad < delivered ? pg.kind : 0u), "%s: first_bad %llu kind %u", what,
        (unsigned long long)res.first_bad, res.bad_kind);
  CHECK(res.bytes == want.size(), "%s: bytes %llu, not %zu", what, (unsigned long long)res.bytes, want.size());
  CHECK(brotli_amd_undba_keep(sg, res.bytes) == keep, "%s: keep", what);
  std::vector<BrotliAmdUndbaLast> lasts(items, BrotliAmdUndbaLast{0u, 0u, 0u});
  Bytes string(string_cap), carried(carry_cap);
  const uint64_t suffixes = src.addr() + res.consumed_p + res.consumed_s;
  if (keep != 0u) {
    for (uint64_t j : order) {
      const BrotliAmdUndbaHostItem it = item_of(j);
      const BrotliAmdUndbaHostLens lens = brotli_amd_undba_host_lens(it, res.first_bad);
      sums_in(j, it.lo, &bytes_in, &suffix_in);
      lasts[j] = brotli_amd_undba_host_a(data.addr(), keep, suffixes, res.data_avail, lens.p.data(), lens.s.data(), (uint32_t)lens.p.size(), bytes_in, suffix_in, string.data(), string_cap);
    }
    brotli_amd_undba_host_b(data.addr(), keep, lasts.data(), items, carried.data(), carry_cap);
    for (uint64_t j : order) {
      if (j == 0u) continue;
      const BrotliAmdUndbaHostItem it = item_of(j);
      const BrotliAmdUndbaHostLens lens = brotli_amd_undba_host_lens(it, res.first_bad);
      sums_in(j, it.lo, &bytes_in, &suffix_in);
      brotli_amd_undba_host_c(data.addr(), keep, lasts[j - 1u], lens.p.data(), lens.s.data(), (uint32_t)lens.p.size(), bytes_in);
    }
  }
  size_t at; uint8_t is, must;
  // the suffix bytes that were cut off read as 0: they are the last `cut` bytes of the suffixes, which end the last strings
  const size_t suffix_total = (size_t)res.suffix_bytes, missing = suffix_total > res.data_avail ? suffix_total - (size_t)res.data_avail : 0u;
  CHECK(((res.data_status & BROTLI_AMD_UNDBA_DATA_SHORT) != 0u) == (missing != 0u), "%s: SHORT", what);
  // (the missing bytes are the last of the suffixes: byte p of the data is one of them where its suffix byte lies at or behind data_avail)
  std::vector<uint8_t> zero(want.size(), 0);
  if (missing != 0u) {
    uint64_t q = 0, at_e = 0;
    for (uint64_t e = 0; e < delivered && e < pg.want.size(); e++) {
      const uint64_t pe = e ? (uint64_t)pg.prefixes[e] : 0u, len_e = pg.want[e].size();
      for (uint64_t k = 0; k < len_e; k++) {
        if (k < pe) zero[at_e + k] = zero[at_e - pg.want[e - 1u].size() + k];
        else zero[at_e + k] = q + (k - pe) >= res.data_avail;
      }
      q += len_e - pe; at_e += len_e;
    }
  }
  CHECK(data.holds([&](size_t p) { return zero[p] ? (uint8_t)0 : (uint8_t)want[p]; }, &at, &is, &must), "%s: data byte %zu is %u, not %u", what, at, is, must);
  CHECK(offsets.holds([&](size_t p) {
          const uint64_t v = ends_only ? ends[p / ow] : p / ow == 0u ? 1000u : ends[p / ow - 1u];
          return (uint8_t)(v >> (8u * (p % ow)));
        }, &at, &is, &must), "%s: offsets byte %zu is %u, not %u", what, at, is, must);
}

int main() {
  // batch.h's second example, by hand
  {
    Page pg;
    const uint8_t body[] = {0x80, 1, 4, 2, 0, 4, 0, 0, 0, 0, 0x80, 1, 4, 2, 6, 3, 0, 0, 0, 0, 'a', 'b', 'c', 'd'};
    pg.body.assign(body, body + sizeof(body)); pg.want = {"abc", "abd"}; pg.prefixes = {0, 2}; pg.first_bad = ~(uint64_t)0; pg.kind = 0;
    run(pg, 0u, 2u, 100u, 0u, 32u, false, 4096u, 32768u, "abc abd");
    run(pg, 0u, 5u, 4u, BROTLI_AMD_UNDBA_OFFSETS64, 32u, true, 1u, 1u, "abc abd cut");
  }
  uint32_t runs = 0;
  for (uint32_t round = 0; round < 60u; round++) {
    const size_t n = (size_t[]){0u, 1u, 2u, 32u, 33u, 34u, 65u, 97u, 200u, 330u}[round % 10u];
    const Strings strings = make_strings(n);
    const uint32_t kind = 1u + round % 3u;
    const size_t bad_at = round % 4u == 3u && n != 0u ? rnd() % n : ~(size_t)0;
    const Page pg = make_page(strings, bad_at, kind);
    for (uint32_t item : {32u, 64u, 96u})
      for (uint32_t caps : {0u, 1u, 2u}) {
        const uint64_t cap = std::max<uint64_t>(1u, caps == 0u ? n : caps == 1u ? (n ? n - 1u : 0u) : n + 5u);
        const uint32_t flags = (rnd() % 2u ? BROTLI_AMD_UNDBA_OFFSETS64 : 0u) | (rnd() % 3u == 0u ? BROTLI_AMD_UNDBA_ENDS_ONLY : 0u);
        const uint32_t string_cap = (uint32_t[]){8u, 24u, 4096u}[rnd() % 3u], carry_cap = (uint32_t[]){8u, 24u, 4096u}[rnd() % 3u];
        const uint64_t data_cap = rnd() % 3u ? ~(uint64_t)0 : rnd() % 400u;
        const size_t cut = bad_at == ~(size_t)0 && rnd() % 5u == 0u && n > 2u ? 1u + rnd() % 3u : 0u;   // (the bytes that are missing read as 0: such a run is judged beside the data alone)
        run(pg, std::min(cut, pg.body.size()), cap, data_cap, flags, item, (rnd() & 1u) != 0u, string_cap, carry_cap, "table");
        runs++;
      }
  }
  if (failures) { std::printf("undba_san: %d failures\n", failures); return 1; }
  std::printf("undba_san: ok (%u runs)\n", runs);
  return 0;
}
