// undict_san.cpp -- the undict lookup and item functions (csrc/brotli_undict.h) on unrle's walk (csrc/brotli_unrle.h) under AddressSanitizer and
// UBSan, as a program of its own:
//   g++ -std=c++17 -fsanitize=address,undefined -I include -I rust-brotli-decompressor_amd/csrc tests/tools/undict_san.cpp
// The walk and then the items, with items of 8, 24 and 40 elements and the device's own, forwards or backwards, against a serial decoder of its
// own.  Every field width 0 .. 32 with EVERY element width; segments put together from seeded runs of both kinds, whole, cut, and with seeded
// bytes behind them; the width byte; capacities of 0, m - 1, m and m + 5; dictionaries of 0, 1, a few and 2^k entries, so that none, some and
// all indices are out of range -- RLE values of up to 0xFFFFFFFF and 32-bit fields against a dictionary of a few entries among them: an index
// that were made an address would leave the block by gigabytes.  Every source and every dictionary lies in a heap block of EXACTLY the
// sixteen-byte words its span touches, at every skew, every destination in one of the words its min(m, cap) elements touch: a load or a store
// one word too far would be reported; the destination's bytes beside the elements must keep their pattern.  Exits 0 when everything agreed.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "brotli_device_abi.h"
#include "brotli_undict.h"
#include "san_block.h"

static uint32_t g_seed = 2031u;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

typedef SanBlock Block;
typedef std::vector<uint8_t> Bytes;

struct Want { std::vector<uint64_t> idx; BrotliAmdUndictResult res; };

// the contract of include/brotli/batch.h, one byte after the other; at most `keep` indices are kept
static Want expect(const uint8_t* s, size_t len, uint32_t k, uint32_t flags, uint64_t keep) {
  Want out;
  out.res = BrotliAmdUndictResult{0u, 0u, 0u, BROTLI_AMD_UNRLE_OK, k, 0u, ~(uint64_t)0};
  size_t off = 0;
  if (flags & BROTLI_AMD_UNDICT_WIDTH_BYTE) {
    out.res.bits = len ? s[0] : 0u;
    if (!len || out.res.bits > 32u) { out.res.status = BROTLI_AMD_UNRLE_BAD_WIDTH; return out; }
    k = out.res.bits; off = 1;
  }
  while (off < len) {
    uint64_t h = 0;
    uint32_t i = 0, stop = 0;
    for (;;) {
      if (off + i >= len) { stop = BROTLI_AMD_UNRLE_TRUNCATED; break; }
      const uint8_t b = s[off + i];
      h |= (uint64_t)(b & 0x7Fu) << (7u * i);
      i++;
      if (b < 0x80u) break;
      if (i == 5u) { stop = BROTLI_AMD_UNRLE_BAD_HEADER; break; }
    }
    if (!stop && (h >> 1) == 0u) stop = BROTLI_AMD_UNRLE_ZERO_RUN;
    if (stop) { out.res.status = stop; break; }
    const size_t at = off + i;
    const uint64_t c = h >> 1, have = len - at;
    if (h & 1u) {
      const uint64_t need = c * k, m = need <= have ? 8u * c : have * 8u / k;
      for (uint64_t j = 0; j < m && out.idx.size() < keep; j++) {
        uint64_t v = 0;
        for (uint32_t t = 0; t < k; t++) { const uint64_t bit = j * k + t; v |= (uint64_t)((s[at + bit / 8u] >> (bit % 8u)) & 1u) << t; }
        out.idx.push_back(v);
      }
      out.res.count += m; out.res.runs += m ? 1u : 0u;
      if (need > have) { out.res.status = BROTLI_AMD_UNRLE_TRUNCATED; off = len; break; }
      off = at + need;
    } else {
      const uint32_t nb = (k + 7u) / 8u;
      if (nb > have) { out.res.status = BROTLI_AMD_UNRLE_TRUNCATED; break; }
      uint64_t v = 0;
      for (uint32_t t = 0; t < nb; t++) v |= (uint64_t)s[at + t] << (8u * t);
      for (uint64_t j = 0; j < c && out.idx.size() < keep; j++) out.idx.push_back(v);
      out.res.count += c; out.res.runs++;
      off = at + nb;
    }
  }
  out.res.consumed = off;
  return out;
}

static void put_header(Bytes* out, uint64_t h, uint32_t pad) {
  Bytes b;
  do { b.push_back((uint8_t)(h & 0x7Fu)); h >>= 7; } while (h);
  while (b.size() < pad && b.size() < 5u) b.push_back(0u);
  for (size_t i = 0; i + 1u < b.size(); i++) b[i] |= 0x80u;
  out->insert(out->end(), b.begin(), b.end());
}

// seeded runs of both kinds that hold about `values` values: seeded payload bytes, so the indices spread over all of 2^k, and the RLE values
// over all of their bytes
static Bytes runs(uint32_t k, uint32_t values, bool width_byte) {
  Bytes out;
  if (width_byte) out.push_back((uint8_t)k);
  for (uint32_t have = 0; have < values;) {
    const uint32_t pad = (rnd() % 4u) ? 0u : 1u + rnd() % 5u;
    if (rnd() & 1u) {
      const uint32_t g = 1u + rnd() % 5u;
      put_header(&out, (uint64_t)g << 1 | 1u, pad);
      for (uint32_t i = 0; i < g * k; i++) out.push_back((uint8_t)rnd());
      have += 8u * g;
    } else {
      const uint32_t c = 1u + rnd() % ((rnd() % 8u) ? 12u : 90u);
      put_header(&out, (uint64_t)c << 1, pad);
      for (uint32_t i = 0; i < (k + 7u) / 8u; i++) out.push_back((rnd() & 3u) ? (uint8_t)rnd() : 0xFFu);
      have += c;
    }
  }
  return out;
}

static unsigned long long g_segments = 0, g_bad = 0, g_good = 0;

// cap_kind: 0: cap 0, 1: m - 1, 2: m, 3: m + 5; D: the dictionary's entries
static int one(const Bytes& bytes, uint32_t k, uint32_t w, uint32_t flags, uint64_t D, uint32_t ss, uint32_t ds, uint32_t ts, uint32_t item_elems, uint32_t cap_kind,
               bool backwards) {
  Block s(bytes.size(), ss);
  s.fill_random(rnd);
  for (size_t i = 0; i < bytes.size(); i++) s.at()[i] = bytes[i];
  Block t((size_t)(D * w), ts);
  t.fill_random(rnd);
  const uint64_t m = expect(s.at(), s.len, k, flags, 0u).res.count;
  const uint64_t cap = cap_kind == 0u ? 0u : cap_kind == 1u ? (m ? m - 1u : 0u) : cap_kind == 2u ? m : m + 5u;
  const uint64_t kept = m < cap ? m : cap;
  if (kept > (1u << 22)) return 0;   // (seeded bytes may announce a run of a length nobody wants to see expanded here)
  Want want = expect(s.at(), s.len, k, flags, kept);
  std::vector<uint64_t> elems(want.idx.size(), 0u);
  for (size_t e = 0; e < want.idx.size(); e++) {
    if (want.idx[e] >= D) { want.res.bad++; if (e < want.res.first_bad) want.res.first_bad = e; continue; }
    for (uint32_t j = 0; j < w; j++) elems[e] |= (uint64_t)t.at()[want.idx[e] * w + j] << (8u * j);
  }
  g_bad += want.res.bad; g_good += elems.size() - want.res.bad;
  Block d((size_t)(kept * w), ds);
  d.fill_pattern();
  const BrotliAmdUndictSeg sg = {s.at(), d.at(), s.len, cap, 0u, w, flags & BROTLI_AMD_UNDICT_WIDTH_BYTE ? 0xEEu : k, flags, 0u, t.at(), D};
  const uint64_t items = brotli_amd_unrle_items(cap, item_elems);
  if (items > (1u << 22)) return 0;
  std::vector<BrotliAmdUnrleCheckpoint> ckpts((size_t)items, BrotliAmdUnrleCheckpoint{BROTLI_AMD_UNRLE_NONE, BROTLI_AMD_UNRLE_NONE});
  BrotliAmdUndictResult got = brotli_amd_undict_host_walk(sg, item_elems, ckpts.data());
  for (uint64_t i = 0; i < items; i++) { const uint64_t j = backwards ? items - 1u - i : i; brotli_amd_undict_host_item(sg, &got, ckpts[(size_t)j], j, item_elems); }
  g_segments++;
  if (got.count != want.res.count || got.consumed != want.res.consumed || got.runs != want.res.runs || got.status != want.res.status || got.bits != want.res.bits ||
      got.bad != want.res.bad || got.first_bad != want.res.first_bad) {
    std::fprintf(stderr, "k %u width %u flags %u length %zu D %llu skews %u %u %u: result %llu %llu %llu %u %u %llu %llu, not %llu %llu %llu %u %u %llu %llu\n", k, w, flags,
                 s.len, (unsigned long long)D, ss, ds, ts, (unsigned long long)got.count, (unsigned long long)got.consumed, (unsigned long long)got.runs, got.status,
                 got.bits, (unsigned long long)got.bad, (unsigned long long)got.first_bad, (unsigned long long)want.res.count, (unsigned long long)want.res.consumed,
                 (unsigned long long)want.res.runs, want.res.status, want.res.bits, (unsigned long long)want.res.bad, (unsigned long long)want.res.first_bad);
    return 1;
  }
  size_t i = 0;
  uint8_t is = 0, must = 0;
  if (d.holds([&](size_t p) { return (uint8_t)(elems[p / w] >> (8u * (p % w))); }, &i, &is, &must)) return 0;
  std::fprintf(stderr, "k %u width %u flags %u length %zu D %llu skews %u %u %u item %u: byte %zu is %02x, not %02x\n", k, w, flags, s.len, (unsigned long long)D, ss, ds,
               ts, item_elems, i, is, must);
  return 1;
}

// a dictionary's entries for fields of k bits: none, one, a few, half of the indices, all of them
static uint64_t entries_for(uint32_t k, uint32_t pick) {
  const uint64_t all = (uint64_t)1 << (k < 12u ? k : 12u);
  switch (pick % 5u) {
    case 0u: return 0u;
    case 1u: return 1u;
    case 2u: return 3u + rnd() % 5u;
    case 3u: return all / 2u + 1u;
    default: return all;
  }
}

int main() {
  const uint32_t item_sizes[4] = {8u, 24u, 40u, BROTLI_AMD_UNRLE_ITEM_ELEMS};
  for (uint32_t k = 0; k <= 32u; k++) {
    for (uint32_t w : {1u, 2u, 4u, 8u}) {
      for (uint32_t wb = 0; wb < 2u; wb++) {
        const Bytes whole = runs(k, 300u, wb != 0u);
        // whole, and cut
        for (uint32_t r = 0; r < 10u; r++)
          if (int e = one(whole, k, w, wb, entries_for(k, r), rnd() & 15u, rnd() & 15u, rnd() & 15u, item_sizes[r & 3u], r & 3u, (r & 4u) != 0u)) return e;
        for (size_t cut = 0; cut < whole.size(); cut += cut < 24u ? 1u : 1u + rnd() % 60u)
          if (int e = one(Bytes(whole.begin(), whole.begin() + cut), k, w, wb, entries_for(k, rnd()), rnd() & 15u, rnd() & 15u, rnd() & 15u, item_sizes[rnd() & 3u],
                          1u + rnd() % 3u, (rnd() & 1u) != 0u)) return e;
        // seeded bytes behind a few runs, and alone
        for (uint32_t r = 0; r < 8u; r++) {
          Bytes b = r < 5u ? runs(k, 20u, wb != 0u) : Bytes();
          for (uint32_t i = 0, n = rnd() % 24u; i < n; i++) b.push_back((uint8_t)((rnd() & 3u) ? rnd() : 0x80u | rnd()));
          if (int e = one(b, k, w, wb, entries_for(k, rnd()), rnd() & 15u, rnd() & 15u, rnd() & 15u, item_sizes[rnd() & 3u], 2u + (rnd() & 1u), (rnd() & 1u) != 0u)) return e;
        }
      }
    }
  }
  // every skew of the dictionary with every skew of the destination, at every width
  for (uint32_t ts = 0; ts < 16u; ts++)
    for (uint32_t ds = 0; ds < 16u; ds++) {
      const uint32_t w = 1u << ((ts + ds) & 3u), k = 1u + rnd() % 10u;
      if (int e = one(runs(k, 40u + rnd() % 100u, false), k, w, 0u, ((uint64_t)1 << k) - (ds & 1u), rnd() & 15u, ds, ts, item_sizes[(ts ^ ds) & 3u], 1u + (ds & 1u) * 2u,
                      (ts & 1u) != 0u)) return e;
    }
  // far-out indices: RLE values of 0xFFFFFFFF and fields of 32 bits against a dictionary of three entries
  for (uint32_t w : {1u, 2u, 4u, 8u}) {
    Bytes b;
    put_header(&b, 6u << 1, 0u); for (int i = 0; i < 4; i++) b.push_back(0xFFu);
    put_header(&b, 1u << 1 | 1u, 0u); for (int i = 0; i < 32; i++) b.push_back((uint8_t)(i % 4 == 3 ? 0x80u | rnd() : rnd()));
    put_header(&b, 3u << 1, 0u); b.push_back(2u); b.push_back(0u); b.push_back(0u); b.push_back(0u);
    for (uint32_t ts = 0; ts < 16u; ts += 5u)
      if (int e = one(b, 32u, w, 0u, 3u, 1u, 2u, ts, 8u, 2u, false)) return e;
  }
  // a width byte that is none, and no bytes at all
  for (uint32_t w : {1u, 2u, 4u, 8u}) {
    if (int e = one(Bytes{33u, 0x10u, 0x05u}, 0u, w, 1u, 4u, 3u, 5u, 7u, 8u, 3u, false)) return e;
    if (int e = one(Bytes(), 3u, w, 1u, 4u, 0u, 0u, 0u, 8u, 3u, false)) return e;
    if (int e = one(Bytes(), 3u, w, 0u, 0u, 0u, 0u, 0u, 8u, 3u, false)) return e;
  }
  if (g_bad == 0u || g_good == 0u) { std::fprintf(stderr, "no bad or no good index was seen\n"); return 1; }
  std::printf("%llu segments\n", g_segments);
  return 0;
}
