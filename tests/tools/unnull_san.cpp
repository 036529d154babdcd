// unnull_san.cpp -- the unnull prefix, mask, rank and validity functions (csrc/brotli_unnull.h) on unrle's walk (csrc/brotli_unrle.h) under
// AddressSanitizer and UBSan, as a program of its own:
//   g++ -std=c++17 -fsanitize=address,undefined -I include -I rust-brotli-decompressor_amd/csrc tests/tools/unnull_san.cpp
// The walk, the counts, the carries and the expansion, with items of 8, 24 and 40 slots and the device's own, forwards or backwards, against a
// serial decoder of its own.  Field widths 0 .. 3, 8, 9 and 32 with every element width; levels put together from seeded runs of both kinds,
// whole, cut, and with seeded bytes behind them; no flags, the length prefix, and the prefix with the values behind the levels; capacities of
// 0, m - 1, m and m + 5; exactly the present slots' values, one fewer, none and more.  Every source and every values array lies in a heap
// block of EXACTLY the sixteen-byte words its span touches, at every skew, every destination and every bitmap in one of the words its slots
// and its ceil(m / 8) bytes touch: a load or a store one word too far would be reported; the bytes beside them must keep their pattern.
// Exits 0 when everything agreed.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "brotli_device_abi.h"
#include "brotli_unnull.h"
#include "san_block.h"

static uint32_t g_seed = 4051u;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

typedef SanBlock Block;
typedef std::vector<uint8_t> Bytes;

struct Want { std::vector<uint64_t> lv; BrotliAmdUnrleResult res; };

// unrle's contract of include/brotli/batch.h, one byte after the other; at most `keep` levels are kept
static Want expect(const uint8_t* s, size_t len, uint32_t k, uint64_t keep) {
  Want out;
  out.res = BrotliAmdUnrleResult{0u, 0u, 0u, BROTLI_AMD_UNRLE_OK, k};
  size_t off = 0;
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
      for (uint64_t j = 0; j < m && out.lv.size() < keep; j++) {
        uint64_t v = 0;
        for (uint32_t t = 0; t < k; t++) { const uint64_t bit = j * k + t; v |= (uint64_t)((s[at + bit / 8u] >> (bit % 8u)) & 1u) << t; }
        out.lv.push_back(v);
      }
      out.res.count += m; out.res.runs += m ? 1u : 0u;
      if (need > have) { out.res.status = BROTLI_AMD_UNRLE_TRUNCATED; off = len; break; }
      off = at + need;
    } else {
      const uint32_t nb = (k + 7u) / 8u;
      if (nb > have) { out.res.status = BROTLI_AMD_UNRLE_TRUNCATED; break; }
      uint64_t v = 0;
      for (uint32_t t = 0; t < nb; t++) v |= (uint64_t)s[at + t] << (8u * t);
      for (uint64_t j = 0; j < c && out.lv.size() < keep; j++) out.lv.push_back(v);
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

// seeded runs of both kinds that hold about `values` levels, of which about one in `nulls` is not `level` (0: none is, 1: every one is): short
// and long runs, so that many runs fall into a lane's 16 slots and single runs span lanes, bytes and items
static Bytes runs(uint32_t k, uint32_t level, uint32_t values, uint32_t nulls) {
  Bytes out;
  const uint64_t top = k ? (((uint64_t)1 << k) - 1u) : 0u;
  auto pick = [&]() -> uint64_t { return nulls == 1u || (nulls && rnd() % nulls == 0u) ? (level + 1u + rnd() % 3u) & top : level; };
  for (uint32_t have = 0; have < values;) {
    const uint32_t pad = (rnd() % 4u) ? 0u : 1u + rnd() % 5u;
    if (rnd() & 1u) {
      const uint32_t g = 1u + rnd() % 5u;
      put_header(&out, (uint64_t)g << 1 | 1u, pad);
      uint64_t acc = 0; uint32_t nbits = 0;
      for (uint32_t i = 0; i < 8u * g; i++) {
        uint64_t v = pick();
        for (uint32_t t = 0; t < k; t++) { acc |= ((v >> t) & 1u) << nbits; if (++nbits == 8u) { out.push_back((uint8_t)acc); acc = 0; nbits = 0; } }
      }
      have += 8u * g;
    } else {
      const uint32_t c = 1u + rnd() % ((rnd() % 4u) ? 12u : 90u);
      put_header(&out, (uint64_t)c << 1, pad);
      uint64_t v = (rnd() % 16u) ? pick() : 0xFFFFFFFFu;   // (an RLE value is not masked)
      for (uint32_t i = 0; i < (k + 7u) / 8u; i++) out.push_back((uint8_t)(v >> (8u * i)));
      have += c;
    }
  }
  return out;
}

static unsigned long long g_segments = 0, g_present = 0, g_null = 0, g_missing = 0, g_bad_length = 0;

// levels: the runs' bytes; flags: 0, the prefix, the prefix and the values behind; prefix_off: added to the true L (not 0: BAD_LENGTH where it
// leaves the segment); cap_kind: 0: cap 0, 1: m - 1, 2: m, 3: m + 5; v_kind: 0: the present slots' values, 1: one fewer, 2: none, 3: five more
static int one(const Bytes& levels, uint32_t k, uint32_t level, uint32_t w, uint32_t flags, int prefix_off, uint32_t ss, uint32_t ds, uint32_t vs, uint32_t bs,
               uint32_t item_elems, uint32_t cap_kind, uint32_t v_kind, bool backwards, bool bitmap, uint32_t left_over) {
  const bool prefix = (flags & BROTLI_AMD_UNNULL_LENGTH_PREFIX) != 0u, follow = (flags & BROTLI_AMD_UNNULL_VALUES_FOLLOW) != 0u;
  if (expect(levels.data(), levels.size(), k, 0u).res.count > (1u << 20)) return 0;   // (seeded bytes may announce a run of a length nobody wants to see expanded here)
  const Want all = expect(levels.data(), levels.size(), k, 1u << 20);
  uint64_t present_all = 0;
  for (uint64_t v : all.lv) present_all += v == level;
  uint64_t V = v_kind == 0u ? present_all : v_kind == 1u ? (present_all ? present_all - 1u : 0u) : v_kind == 2u ? 0u : present_all + 5u;
  // the segment
  Bytes seg;
  if (prefix) { const uint32_t L = (uint32_t)((int64_t)levels.size() + prefix_off); for (uint32_t i = 0; i < 4u; i++) seg.push_back((uint8_t)(L >> (8u * i))); }
  seg.insert(seg.end(), levels.begin(), levels.end());
  Bytes vals((size_t)(V * w));
  for (uint8_t& b : vals) b = (uint8_t)(1u + rnd() % 255u);
  if (follow) { seg.insert(seg.end(), vals.begin(), vals.end()); for (uint32_t i = 0; i < left_over % w; i++) seg.push_back(0xEEu); }
  Block s(seg.size(), ss);
  s.fill_random(rnd);
  for (size_t i = 0; i < seg.size(); i++) s.at()[i] = seg[i];
  Block t(follow ? 0u : vals.size(), vs);
  t.fill_random(rnd);
  for (size_t i = 0; !follow && i < vals.size(); i++) t.at()[i] = vals[i];
  // what the contract says
  BrotliAmdUnnullResult want = {0u, 0u, 0u, BROTLI_AMD_UNRLE_OK, k, 0u, 0u, follow ? 0u : V};
  std::vector<uint64_t> lv;
  uint64_t cap = 0;
  const uint64_t L = prefix && seg.size() >= 4u ? (uint64_t)seg[0] | (uint64_t)seg[1] << 8 | (uint64_t)seg[2] << 16 | (uint64_t)seg[3] << 24 : 0u;
  if (prefix && (seg.size() < 4u || L > seg.size() - 4u)) {
    want.status = BROTLI_AMD_UNNULL_BAD_LENGTH;
    cap = cap_kind == 0u ? 0u : 5u;
    g_bad_length++;
  } else {
    const uint8_t* r0 = s.at() + (prefix ? 4u : 0u);
    const size_t rlen = prefix ? (size_t)L : seg.size();
    const uint64_t m = expect(r0, rlen, k, 0u).res.count;
    if (m > (1u << 20)) return 0;   // (a length that reaches into the values: seeded bytes again)
    cap = cap_kind == 0u ? 0u : cap_kind == 1u ? (m ? m - 1u : 0u) : cap_kind == 2u ? m : m + 5u;
    Want got = expect(r0, rlen, k, m < cap ? m : cap);
    lv = got.lv;
    want.count = got.res.count; want.consumed = got.res.consumed + (prefix ? 4u : 0u); want.runs = got.res.runs; want.status = got.res.status;
    if (follow) want.values = want.status == BROTLI_AMD_UNRLE_OK ? (seg.size() - want.consumed) / w : 0u;
  }
  const uint64_t kept = lv.size();
  const uint8_t* table = follow ? s.at() + want.consumed : t.at();
  std::vector<uint64_t> slots(kept, 0u);
  Bytes bits((size_t)((kept + 7u) / 8u), 0u);
  uint64_t rank = 0;
  for (size_t e = 0; e < kept; e++) {
    if (lv[e] != level) { g_null++; continue; }
    bits[e >> 3] |= (uint8_t)(1u << (e & 7u));
    want.present++;
    if (rank < want.values) { for (uint32_t j = 0; j < w; j++) slots[e] |= (uint64_t)table[rank * w + j] << (8u * j); g_present++; }
    else { want.missing++; g_missing++; }
    rank++;
  }
  Block d((size_t)(kept * w), ds), b(bitmap ? bits.size() : 0u, bs);
  d.fill_pattern();
  b.fill_pattern();
  const BrotliAmdUnnullSeg sg = {s.at(), d.at(), s.len, cap, 0u, w, k, flags, level, follow ? nullptr : t.at(), follow ? 0xDEADu : V, bitmap ? b.at() : nullptr};
  const uint64_t items = brotli_amd_unrle_items(cap, item_elems);
  if (items > (1u << 20)) return 0;
  std::vector<BrotliAmdUnrleCheckpoint> ckpts((size_t)items, BrotliAmdUnrleCheckpoint{BROTLI_AMD_UNRLE_NONE, BROTLI_AMD_UNRLE_NONE});
  BrotliAmdUnnullRuns where;
  BrotliAmdUnnullResult got = brotli_amd_unnull_host_walk(sg, item_elems, ckpts.data(), &where);
  std::vector<uint32_t> masks((item_elems + 15u) / 16u);
  std::vector<BrotliAmdUndeltaTile> tiles((size_t)items);
  auto order = [&](uint64_t i) { return backwards ? items - 1u - i : i; };
  for (uint64_t i = 0; i < items; i++) {
    const uint64_t j = order(i);
    std::fill(masks.begin(), masks.end(), 0u);
    tiles[(size_t)j] = brotli_amd_unnull_host_count(sg, where, got, ckpts[(size_t)j], j, item_elems, masks.data());
  }
  std::vector<uint64_t> carries((size_t)items);
  BrotliAmdUndeltaPair out = {0u, 0u};
  for (size_t j = 0; j < tiles.size(); j++) {
    carries[j] = brotli_amd_undelta_carry_in(out.sum, tiles[j]);
    out = brotli_amd_undelta_combine(out, brotli_amd_undelta_tile_pair(tiles[j]));
  }
  for (uint64_t i = 0; i < items; i++) {
    const uint64_t j = order(items - 1u - i);
    std::fill(masks.begin(), masks.end(), 0u);
    brotli_amd_unnull_host_expand(sg, where, &got, ckpts[(size_t)j], j, item_elems, carries[(size_t)j], masks.data());
  }
  g_segments++;
  if (got.count != want.count || got.consumed != want.consumed || got.runs != want.runs || got.status != want.status || got.bits != want.bits ||
      got.present != want.present || got.missing != want.missing || got.values != want.values) {
    std::fprintf(stderr, "k %u level %u width %u flags %u length %zu V %llu cap %llu item %u: result %llu %llu %llu %u %u %llu %llu %llu, not %llu %llu %llu %u %u %llu %llu %llu\n", k,
                 level, w, flags, s.len, (unsigned long long)V, (unsigned long long)cap, item_elems, (unsigned long long)got.count, (unsigned long long)got.consumed,
                 (unsigned long long)got.runs, got.status, got.bits, (unsigned long long)got.present, (unsigned long long)got.missing, (unsigned long long)got.values,
                 (unsigned long long)want.count, (unsigned long long)want.consumed, (unsigned long long)want.runs, want.status, want.bits, (unsigned long long)want.present,
                 (unsigned long long)want.missing, (unsigned long long)want.values);
    return 1;
  }
  size_t i = 0;
  uint8_t is = 0, must = 0;
  if (!d.holds([&](size_t p) { return (uint8_t)(slots[p / w] >> (8u * (p % w))); }, &i, &is, &must)) {
    std::fprintf(stderr, "k %u level %u width %u flags %u length %zu skews %u %u %u %u item %u: slot byte %zu is %02x, not %02x\n", k, level, w, flags, s.len, ss, ds, vs, bs,
                 item_elems, i, is, must);
    return 1;
  }
  if (!b.holds([&](size_t p) { return bits[p]; }, &i, &is, &must)) {
    std::fprintf(stderr, "k %u level %u width %u flags %u length %zu skews %u %u %u %u item %u: validity byte %zu is %02x, not %02x\n", k, level, w, flags, s.len, ss, ds, vs,
                 bs, item_elems, i, is, must);
    return 1;
  }
  return 0;
}

int main() {
  const uint32_t item_sizes[4] = {8u, 24u, 40u, BROTLI_AMD_UNRLE_ITEM_ELEMS};
  const uint32_t flag_sets[3] = {0u, BROTLI_AMD_UNNULL_LENGTH_PREFIX, BROTLI_AMD_UNNULL_LENGTH_PREFIX | BROTLI_AMD_UNNULL_VALUES_FOLLOW};
  for (uint32_t k : {0u, 1u, 2u, 3u, 8u, 9u, 32u}) {
    const uint32_t top = k >= 32u ? 0xFFFFFFFFu : (1u << k) - 1u;
    for (uint32_t level : {0u, top, top / 2u}) {
      for (uint32_t w : {1u, 2u, 4u, 8u}) {
        for (uint32_t nulls : {0u, 1u, 2u, 4u, 50u}) {
          const Bytes whole = runs(k, level, 200u + rnd() % 2200u, nulls);
          for (uint32_t r = 0; r < 8u; r++)
            if (int e = one(whole, k, level, w, flag_sets[r % 3u], 0, rnd() & 15u, rnd() & 15u, rnd() & 15u, rnd() & 15u, item_sizes[r & 3u], r & 3u, (r >> 1) & 3u, (r & 4u) != 0u,
                            r != 5u, rnd()))
              return e;
          // cut, and with seeded bytes behind: every stop
          for (uint32_t r = 0; r < 6u; r++) {
            Bytes b(whole.begin(), whole.begin() + rnd() % (whole.size() < 200u ? whole.size() : 200u));
            if (r & 1u) for (uint32_t i = 0, n = rnd() % 12u; i < n; i++) b.push_back((uint8_t)((rnd() & 3u) ? rnd() : 0x80u | rnd()));
            if (int e = one(b, k, level, w, flag_sets[rnd() % 3u], 0, rnd() & 15u, rnd() & 15u, rnd() & 15u, rnd() & 15u, item_sizes[rnd() & 3u], 1u + rnd() % 3u, rnd() & 3u,
                            (rnd() & 1u) != 0u, true, rnd()))
              return e;
          }
        }
        // the prefix: a length one above the room, one that cuts the runs, and segments of 0 .. 4 bytes
        const Bytes few = runs(k, level, 40u, 3u);
        for (int off : {1, -1, -3, 1000000})
          for (uint32_t f = 1; f < 3u; f++)
            if (int e = one(few, k, level, w, flag_sets[f], f == 2u && off > 0 ? off + 64 : off, rnd() & 15u, rnd() & 15u, rnd() & 15u, rnd() & 15u, 8u, 2u, 0u, false, true, rnd()))
              return e;
      }
    }
  }
  // every skew of the bitmap with every skew of the destination, m % 8 in 0 .. 7
  for (uint32_t bs = 0; bs < 16u; bs++)
    for (uint32_t ds = 0; ds < 16u; ds++) {
      const uint32_t w = 1u << ((bs + ds) & 3u);
      Bytes b = runs(1u, 1u, 130u + bs, 3u);
      put_header(&b, (uint64_t)(1u + (ds & 7u)) << 1, 0u); b.push_back(1u);
      if (int e = one(b, 1u, 1u, w, flag_sets[(bs + ds) % 3u], 0, rnd() & 15u, ds, rnd() & 15u, bs, item_sizes[(bs ^ ds) & 3u], 2u, ds & 1u, (bs & 1u) != 0u, true, rnd())) return e;
    }
  for (uint32_t len = 0; len < 4u; len++) {   // a prefix that is cut
    const Block s(len, 3u);
    for (size_t i = 0; i < len; i++) s.at()[i] = 0u;
    const BrotliAmdUnnullSeg sg = {s.at(), nullptr, len, 0u, 0u, 4u, 1u, BROTLI_AMD_UNNULL_LENGTH_PREFIX, 1u, nullptr, 0u, nullptr};
    BrotliAmdUnnullRuns where;
    const BrotliAmdUnnullResult got = brotli_amd_unnull_host_walk(sg, 8u, nullptr, &where);
    if (got.status != BROTLI_AMD_UNNULL_BAD_LENGTH || got.count != 0u || got.consumed != 0u) { std::fprintf(stderr, "a prefix of %u bytes: status %u\n", len, got.status); return 1; }
    g_bad_length++;
  }
  if (g_present == 0u || g_null == 0u || g_missing == 0u || g_bad_length == 0u) { std::fprintf(stderr, "no present, null or missing slot, or no bad length, was seen\n"); return 1; }
  std::printf("%llu segments\n", g_segments);
  return 0;
}
