// undlba_san.cpp -- the host phases of csrc/brotli_undlba.h (on undbp's walk and items, csrc/brotli_undbp.h) under AddressSanitizer and UBSan,
// as a program of its own:
//   g++ -std=c++17 -fsanitize=address,undefined -I include -I rust-brotli-decompressor_amd/csrc tests/tools/undlba_san.cpp
// The walk, the items' delta sums, the carries, the items' lengths, the carries of their bytes, the items' offsets and the copy, with items of
// 32, 64 and 96 deltas and the device's own, forwards or backwards, against a serial decoder of its own: the five examples of
// include/brotli/batch.h, and a seeded table of page bodies -- block shapes (128, 4) and (256, 8), strings of 0 .. 40 bytes, negative and
// oversized lengths, bodies cut at seeded places and with bytes left over, capacities of 0, m - 1, m and m + 5, data capacities that cut, both
// offset widths and ENDS_ONLY, seeded skews.  Every source lies in a heap block of EXACTLY the sixteen-byte words its span touches, and so do
// the offsets and the data that a segment delivers: a load or a store one word too far would be reported; the destinations' bytes beside what
// is delivered must keep their pattern.  Exits 0 when everything agreed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <vector>

#include "brotli_device_abi.h"
#include "brotli_undlba.h"
#include "san_block.h"

static uint32_t g_seed = 4099u;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

typedef SanBlock Block;
typedef std::vector<uint8_t> Bytes;

// ---- a serial decoder of the contract: a value after the other, nothing shared with the header under test ----
static uint32_t read_varint(const uint8_t* s, size_t len, size_t off, uint64_t* value, size_t* bytes) {
  uint64_t v = 0;
  for (uint32_t i = 0; i < 10u; i++) {
    if (off + i >= len) return BROTLI_AMD_UNDBP_TRUNCATED;
    const uint8_t b = s[off + i];
    if (i < 9u) v |= (uint64_t)(b & 0x7Fu) << (7u * i); else v |= (uint64_t)(b & 1u) << 63;
    if (!(b & 0x80u)) { *value = v; *bytes = i + 1u; return BROTLI_AMD_UNDBP_OK; }
  }
  return BROTLI_AMD_UNDBP_BAD_HEADER;
}
static uint64_t unzigzag(uint64_t u) { return (u >> 1) ^ (0u - (u & 1u)); }

struct Want { std::vector<uint64_t> ends; BrotliAmdUndlbaResult res; };   // ends: of the first min(count, cap) elements, on a base of 0

static void take(Want* w, uint64_t v, uint64_t e, uint64_t cap) {
  if (e >= cap) return;
  const int64_t L = (int32_t)(uint32_t)v;
  if (L < 0) { w->res.bad++; if (e < w->res.first_bad) w->res.first_bad = e; }
  w->ends.push_back((w->ends.empty() ? 0u : w->ends.back()) + (L < 0 ? 0u : (uint64_t)L));
}
static Want expect(const uint8_t* s, size_t len, uint64_t cap) {
  Want out;
  out.res = BrotliAmdUndlbaResult{0u, 0u, 0u, 0u, BROTLI_AMD_UNDBP_OK, 0u, 0u, BROTLI_AMD_UNDLBA_DATA_OK, 0u, ~(uint64_t)0, 0u, len};
  uint64_t h[4];
  size_t off = 0, nb = 0;
  for (uint32_t i = 0; i < 4u; i++) {
    if (uint32_t st = read_varint(s, len, off, &h[i], &nb)) { out.res.status = st; return out; }
    off += nb;
  }
  const uint64_t B = h[0], M = h[1], N = h[2];
  out.res.declared = N;
  out.res.block_values = B > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)B;
  out.res.miniblocks = M > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)M;
  if (B == 0u || B % 128u || B > 65536u || M == 0u || B % M || (B / M) % 32u) { out.res.status = BROTLI_AMD_UNDBP_BAD_HEADER; return out; }
  out.res.consumed = off; out.res.data_avail = len - off;
  if (N == 0u) return out;
  const uint64_t V = B / M;
  uint64_t v = unzigzag(h[3]), count = 1;
  take(&out, v, 0u, cap);
  while (count < N) {
    uint64_t md = 0;
    if (uint32_t st = read_varint(s, len, off, &md, &nb)) { out.res.status = st; break; }
    const size_t wat = off + nb;
    if (M > len - wat) { out.res.status = BROTLI_AMD_UNDBP_TRUNCATED; break; }
    const uint64_t remaining = N - count, need = (remaining + V - 1u) / V < M ? (remaining + V - 1u) / V : M;
    bool bad = false;
    for (uint64_t j = 0; j < need; j++) bad = bad || s[wat + j] > 64u;
    if (bad) { out.res.status = BROTLI_AMD_UNDBP_BAD_WIDTH; break; }
    md = unzigzag(md);
    size_t pos = wat + (size_t)M;
    uint64_t got = 0;
    for (uint64_t j = 0; j < need && out.res.status == BROTLI_AMD_UNDBP_OK; j++) {
      const uint32_t k = s[wat + j];
      const uint64_t bytes = V * k / 8u;
      uint64_t want = V < remaining - got ? V : remaining - got;
      if (bytes > len - pos) {
        const uint64_t part = (uint64_t)(len - pos) * 8u / k;
        want = part < want ? part : want;
        out.res.status = BROTLI_AMD_UNDBP_TRUNCATED;
      }
      for (uint64_t t = 0; t < want; t++) {
        uint64_t f = 0;
        for (uint32_t bit = 0; bit < k; bit++) {
          const uint64_t at = t * k + bit;
          f |= (uint64_t)((s[pos + at / 8u] >> (at % 8u)) & 1u) << bit;
        }
        v += md + f;
        take(&out, v, count + got + t, cap);
      }
      got += want;
      pos = out.res.status == BROTLI_AMD_UNDBP_OK ? pos + (size_t)bytes : len;
    }
    if (got) out.res.blocks++;
    count += got; off = pos;
    if (out.res.status != BROTLI_AMD_UNDBP_OK) break;
  }
  out.res.count = count; out.res.consumed = off; out.res.data_avail = len - off;
  return out;
}

// ---- page bodies ----
static void put_varint(Bytes* out, uint64_t v) {
  do { out->push_back((uint8_t)((v & 0x7Fu) | (v > 0x7Fu ? 0x80u : 0u))); v >>= 7; } while (v);
}
static uint64_t zigzag(uint64_t v) { return (v << 1) ^ (0u - (v >> 63)); }
// the lengths as a DELTA_BINARY_PACKED stream, every miniblock at the width its fields need, then `data`
static Bytes body(uint32_t B, uint32_t M, const std::vector<uint64_t>& lengths, const Bytes& data) {
  Bytes out;
  const uint32_t V = B / M;
  put_varint(&out, B); put_varint(&out, M); put_varint(&out, lengths.size()); put_varint(&out, lengths.empty() ? 0u : zigzag(lengths[0]));
  for (size_t at = 1; at < lengths.size(); at += B) {
    const size_t n = lengths.size() - at < B ? lengths.size() - at : B;
    int64_t lo = INT64_MAX;
    for (size_t i = 0; i < n; i++) { const int64_t d = (int64_t)(lengths[at + i] - lengths[at + i - 1u]); lo = d < lo ? d : lo; }
    put_varint(&out, zigzag((uint64_t)lo));
    const size_t minis = (n + V - 1u) / V;
    std::vector<uint8_t> widths(M, 0xEEu);
    for (size_t j = 0; j < minis; j++) {
      uint64_t all = 0;
      for (size_t i = j * V; i < n && i < (j + 1u) * V; i++) all |= lengths[at + i] - lengths[at + i - 1u] - (uint64_t)lo;
      widths[j] = (uint8_t)(all ? 64 - __builtin_clzll(all) : 0);
    }
    out.insert(out.end(), widths.begin(), widths.end());
    for (size_t j = 0; j < minis; j++) {
      Bytes payload((size_t)V / 8u * widths[j], 0u);
      for (size_t i = j * V; i < n && i < (j + 1u) * V; i++) {
        const uint64_t f = lengths[at + i] - lengths[at + i - 1u] - (uint64_t)lo;
        for (uint32_t bit = 0; bit < widths[j]; bit++) {
          const size_t p = (i - j * V) * widths[j] + bit;
          payload[p / 8u] |= (uint8_t)(((f >> bit) & 1u) << (p % 8u));
        }
      }
      out.insert(out.end(), payload.begin(), payload.end());
    }
  }
  out.insert(out.end(), data.begin(), data.end());
  return out;
}

static unsigned long long g_segments = 0;

// cap_kind: 0: cap 0, 1: m - 1, 2: m, 3: m + 5; data_kind: 0: no data destination, 1: all, 2: half, 3: a capacity of 0
static int one(const Bytes& bytes, uint32_t flags, uint64_t base, uint32_t ss, uint32_t os, uint32_t ds, uint32_t item_deltas, uint32_t cap_kind, uint32_t data_kind,
               bool backwards, const Want* pinned = nullptr) {
  Block s(bytes.size(), ss);
  s.fill_random(rnd);
  for (size_t i = 0; i < bytes.size(); i++) s.at()[i] = bytes[i];
  const uint64_t count = expect(s.at(), s.len, 0u).res.count;
  const uint64_t cap = cap_kind == 0u ? 0u : cap_kind == 1u ? (count ? count - 1u : 0u) : cap_kind == 2u ? count : count + 5u;
  Want want = expect(s.at(), s.len, cap);
  const uint64_t m = want.ends.size(), total = m ? want.ends.back() : 0u;
  if (cap != 0u) { want.res.bytes = total; want.res.data_status = total <= want.res.data_avail ? BROTLI_AMD_UNDLBA_DATA_OK : BROTLI_AMD_UNDLBA_DATA_SHORT; }
  else { want.res.bad = 0u; want.res.first_bad = ~(uint64_t)0; }
  if (pinned && (pinned->res.count != want.res.count || pinned->res.consumed != want.res.consumed || pinned->res.bad != want.res.bad || pinned->res.first_bad != want.res.first_bad ||
                 pinned->res.bytes != want.res.bytes || pinned->res.data_avail != want.res.data_avail || pinned->res.data_status != want.res.data_status || pinned->ends != want.ends)) {
    std::fprintf(stderr, "an example is not what batch.h says\n");
    return 1;
  }
  const uint32_t ow = (flags & BROTLI_AMD_UNDLBA_OFFSETS64) ? 8u : 4u;
  const bool ends_only = (flags & BROTLI_AMD_UNDLBA_ENDS_ONLY) != 0u;
  const uint64_t slots = cap == 0u ? 0u : m + (ends_only ? 0u : 1u);
  uint64_t keep = total < want.res.data_avail ? total : want.res.data_avail;
  const uint64_t data_cap = data_kind == 1u ? keep + 3u : data_kind == 2u ? keep / 2u : 0u;
  keep = data_kind == 0u || cap == 0u ? 0u : keep < data_cap ? keep : data_cap;
  Block o((size_t)(slots * ow), os), d((size_t)keep, ds);
  o.fill_pattern(); d.fill_pattern();
  const BrotliAmdUndlbaSeg sg = {s.at(), data_kind == 0u ? nullptr : d.at(), s.len, cap, 0u, flags, 0u, o.at(), data_cap, base};
  const uint64_t items = brotli_amd_undbp_items(cap, item_deltas);
  std::vector<BrotliAmdUndbpCheckpoint> ckpts((size_t)items, BrotliAmdUndbpCheckpoint{BROTLI_AMD_UNDBP_NONE, BROTLI_AMD_UNDBP_NONE});
  uint64_t first = 0;
  BrotliAmdUndlbaResult got = brotli_amd_undlba_host_walk(sg, item_deltas, ckpts.data(), &first);
  std::vector<BrotliAmdUndeltaTile> tiles((size_t)items), byte_tiles((size_t)items);
  std::vector<uint64_t> carries((size_t)items), byte_carries((size_t)items);
  auto order = [&](uint64_t i, bool back) { return (size_t)(back ? items - 1u - i : i); };
  auto carry = [&](const std::vector<BrotliAmdUndeltaTile>& t, std::vector<uint64_t>* c) {
    BrotliAmdUndeltaPair run = {0u, 0u};
    for (size_t j = 0; j < t.size(); j++) {
      (*c)[j] = brotli_amd_undelta_carry_in(run.sum, t[j]);
      run = brotli_amd_undelta_combine(run, brotli_amd_undelta_tile_pair(t[j]));
    }
  };
  for (uint64_t i = 0; i < items; i++) { const size_t j = order(i, backwards); tiles[j] = brotli_amd_undlba_host_sum(sg, got, ckpts[j], first, j, item_deltas); }
  carry(tiles, &carries);
  for (uint64_t i = 0; i < items; i++) { const size_t j = order(i, !backwards); byte_tiles[j] = brotli_amd_undlba_host_lengths(sg, &got, ckpts[j], first, j, item_deltas, carries[j]); }
  carry(byte_tiles, &byte_carries);
  BrotliAmdCopySeg copy = {nullptr, nullptr, 0u};
  for (uint64_t i = 0; i < items; i++) { const size_t j = order(i, backwards); brotli_amd_undlba_host_expand(sg, &got, ckpts[j], first, j, item_deltas, carries[j], byte_carries[j], &copy); }
  brotli_amd_undlba_host_copy(copy);
  g_segments++;
  const BrotliAmdUndlbaResult& w = want.res;
  if (got.count != w.count || got.consumed != w.consumed || got.declared != w.declared || got.blocks != w.blocks || got.status != w.status || got.block_values != w.block_values ||
      got.miniblocks != w.miniblocks || got.data_status != w.data_status || got.bad != w.bad || got.first_bad != w.first_bad || got.bytes != w.bytes || got.data_avail != w.data_avail) {
    std::fprintf(stderr, "length %zu flags %u cap %llu item %u: result %llu %llu %u %u bad %llu %llu bytes %llu %llu, not %llu %llu %u %u bad %llu %llu bytes %llu %llu\n", s.len, flags,
                 (unsigned long long)cap, item_deltas, (unsigned long long)got.count, (unsigned long long)got.consumed, got.status, got.data_status, (unsigned long long)got.bad,
                 (unsigned long long)got.first_bad, (unsigned long long)got.bytes, (unsigned long long)got.data_avail, (unsigned long long)w.count, (unsigned long long)w.consumed,
                 w.status, w.data_status, (unsigned long long)w.bad, (unsigned long long)w.first_bad, (unsigned long long)w.bytes, (unsigned long long)w.data_avail);
    return 1;
  }
  size_t i = 0;
  uint8_t is = 0, must = 0;
  auto offset_byte = [&](size_t p) {
    const size_t slot = p / ow + (ends_only ? 1u : 0u);
    const uint64_t v = base + (slot ? want.ends[slot - 1u] : 0u);
    return (uint8_t)(v >> (8u * (p % ow)));
  };
  if (!o.holds(offset_byte, &i, &is, &must)) {
    std::fprintf(stderr, "length %zu flags %u cap %llu item %u skew %u: offsets byte %zu is %02x, not %02x\n", s.len, flags, (unsigned long long)cap, item_deltas, os, i, is, must);
    return 1;
  }
  if (!d.holds([&](size_t p) { return s.at()[want.res.consumed + p]; }, &i, &is, &must)) {
    std::fprintf(stderr, "length %zu flags %u cap %llu item %u skew %u: data byte %zu is %02x, not %02x\n", s.len, flags, (unsigned long long)cap, item_deltas, ds, i, is, must);
    return 1;
  }
  return 0;
}

static Bytes hex(std::initializer_list<int> b) { Bytes out; for (int x : b) out.push_back((uint8_t)x); return out; }

int main() {
  const uint64_t none = ~(uint64_t)0;
  const uint32_t item_sizes[4] = {32u, 64u, 96u, BROTLI_AMD_UNDBP_ITEM_DELTAS};
  // the five examples of include/brotli/batch.h, pinned by hand: (count, consumed, data_status, bad, first_bad, bytes, data_avail), the ends
  struct Example { Bytes bytes; Want want; };
  auto pinned = [](uint64_t count, uint64_t consumed, uint32_t data_status, uint64_t bad, uint64_t first_bad, uint64_t bytes, uint64_t avail, std::vector<uint64_t> ends) {
    Want w;
    w.ends = ends;
    w.res = BrotliAmdUndlbaResult{count, consumed, 0u, 0u, 0u, 0u, 0u, data_status, bad, first_bad, bytes, avail};
    return w;
  };
  const Example examples[5] = {
      {hex({0x80, 0x01, 0x04, 0x04, 0x00, 0x02, 0x00, 0x00, 0x00, 0x00, 0x61, 0x62, 0x62, 0x63, 0x63, 0x63}), pinned(4u, 10u, 0u, 0u, none, 6u, 6u, {0u, 1u, 3u, 6u})},
      {hex({0x80, 0x01, 0x04, 0x01, 0x06, 0x78, 0x79, 0x7a}), pinned(1u, 5u, 0u, 0u, none, 3u, 3u, {3u})},
      {hex({0x80, 0x01, 0x04, 0x01, 0x01, 0x61, 0x62}), pinned(1u, 5u, 0u, 1u, 0u, 0u, 2u, {0u})},
      {hex({0x80, 0x01, 0x04, 0x01, 0x0a, 0x61, 0x62}), pinned(1u, 5u, 1u, 0u, none, 5u, 2u, {5u})},
      {hex({0x80, 0x01, 0x04, 0x00, 0x00}), pinned(0u, 5u, 0u, 0u, none, 0u, 0u, {})},
  };
  for (const Example& ex : examples)
    for (uint32_t flags : {0u, 2u, 4u, 6u})
      for (uint32_t item : item_sizes)
        if (int e = one(ex.bytes, flags, flags ? 0xFFFFFFF0u : 0u, rnd() & 15u, rnd() & 15u, rnd() & 15u, item, 3u, 1u, (rnd() & 1u) != 0u, &ex.want)) return e;
  // a seeded table
  const uint32_t shapes[2][2] = {{128u, 4u}, {256u, 8u}};
  for (uint32_t r = 0; r < 600u; r++) {
    const uint32_t* shape = shapes[r & 1u];
    const uint32_t n = (r % 7u == 0u) ? rnd() % 3u : rnd() % 700u, top = 1u + rnd() % 40u;
    std::vector<uint64_t> lengths;
    Bytes data;
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t L = (rnd() & 3u) ? rnd() % top : 0u;
      lengths.push_back(L);
      for (uint32_t b = 0; b < L; b++) data.push_back((uint8_t)rnd());
    }
    if (n && r % 5u == 1u) lengths[rnd() % n] = (uint64_t)0 - (1u + rnd() % 1000u);          // negative
    if (n && r % 5u == 2u) lengths[rnd() % n] += 1u + rnd() % 100u;                          // the data is short
    if (n && r % 5u == 3u) lengths[rnd() % n] += (uint64_t)(1u + rnd() % 7u) << 32;          // upper bits that are not looked at
    Bytes b = body(shape[0], shape[1], lengths, data);
    if (r % 11u == 4u && !b.empty()) b.resize(rnd() % b.size());                             // cut
    if (r % 11u == 5u) for (uint32_t i = 0, more = 1u + rnd() % 20u; i < more; i++) b.push_back((uint8_t)rnd());   // left over
    const uint32_t flags = (rnd() & 1u ? 2u : 0u) | (rnd() & 1u ? 4u : 0u);
    if (int e = one(b, flags, (rnd() & 1u) ? 0u : 0xFFFFFF00u, rnd() & 15u, rnd() & 15u, rnd() & 15u, item_sizes[rnd() & 3u], rnd() & 3u, rnd() & 3u, (rnd() & 1u) != 0u)) return e;
  }
  // no bytes at all
  if (int e = one(Bytes(), 0u, 0u, 0u, 0u, 0u, 32u, 3u, 1u, false)) return e;
  std::printf("undlba_san: ok, %llu segments\n", g_segments);
  return 0;
}
