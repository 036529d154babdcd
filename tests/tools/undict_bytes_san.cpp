// undict_bytes_san.cpp -- the functions of csrc/brotli_undict_bytes.h on unrle's walk (csrc/brotli_unrle.h) under AddressSanitizer and UBSan, as
// a program of its own:
//   g++ -std=c++17 -fsanitize=address,undefined -I include -I rust-brotli-decompressor_amd/csrc tests/tools/undict_bytes_san.cpp
// The dictionary's walk, the segment's walk, the items' byte counts, the carries and the items' offsets and bytes, with items of 8, 24 and 40
// elements and the device's own, the items and an item's words forwards or backwards, against a serial decoder of its own.  Field widths 0 .. 32;
// segments put together from seeded runs of both kinds, whole and cut; dictionaries of 0, 1, a few and 2^k entries of 0 .. 40 bytes, whole, cut
// at a seeded byte and bounded, so that none, some and all indices are out of range -- RLE values of 0xFFFFFFFF and 32-bit fields against a
// dictionary of three entries among them: an index that were made an address would leave the block by gigabytes --; both offset widths, with
// and without offsets[0]; data capacities of 0, inside, at and above the bytes.  The source, the dictionary, starts[], the offsets and the data
// each lie in a heap block of EXACTLY the sixteen-byte words their span touches, at every skew: a load or a store one word too far would be
// reported; the destinations' bytes beside what is written must keep their pattern.  Exits 0 when everything agreed.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "brotli_device_abi.h"
#include "brotli_undict_bytes.h"
#include "san_block.h"

static uint32_t g_seed = 4051u;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

typedef SanBlock Block;
typedef std::vector<uint8_t> Bytes;

struct Want { std::vector<uint64_t> idx; BrotliAmdUnrleResult res; };

// unrle's contract, one byte after the other; at most `keep` indices are kept
static Want expect(const uint8_t* s, size_t len, uint32_t k, uint32_t flags, uint64_t keep) {
  Want out;
  out.res = BrotliAmdUnrleResult{0u, 0u, 0u, BROTLI_AMD_UNRLE_OK, k};
  size_t off = 0;
  if (flags & BROTLI_AMD_UNDICT_BYTES_WIDTH_BYTE) {
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

// seeded runs of both kinds that hold about `values` values: seeded payload bytes, so the indices spread over all of 2^k
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

// a dictionary of D entries of 0 .. 40 seeded bytes
static Bytes dictionary(uint64_t D) {
  Bytes out;
  for (uint64_t e = 0; e < D; e++) {
    const uint32_t n = (rnd() & 3u) ? rnd() % 9u : rnd() % 41u;
    for (uint32_t j = 0; j < 4u; j++) out.push_back((uint8_t)(n >> (8u * j)));
    for (uint32_t j = 0; j < n; j++) out.push_back((uint8_t)rnd());
  }
  return out;
}

// the dictionary's contract, one entry after the other
struct Parsed { std::vector<Bytes> entries; uint64_t consumed; uint32_t status; };
static Parsed parse(const uint8_t* d, size_t len, uint64_t bound) {
  Parsed p = {{}, 0u, BROTLI_AMD_UNDICT_BYTES_DICT_OK};
  while (p.entries.size() < bound && p.consumed < len) {
    const size_t left = len - (size_t)p.consumed;
    if (left < 4u) { p.status = BROTLI_AMD_UNDICT_BYTES_DICT_CUT; break; }
    const uint8_t* at = d + p.consumed;
    const uint64_t n = (uint64_t)at[0] | (uint64_t)at[1] << 8 | (uint64_t)at[2] << 16 | (uint64_t)at[3] << 24;
    if (n > left - 4u) { p.status = BROTLI_AMD_UNDICT_BYTES_DICT_CUT; break; }
    p.entries.push_back(Bytes(at + 4, at + 4 + n));
    p.consumed += 4u + n;
  }
  return p;
}

static unsigned long long g_segments = 0, g_bad = 0, g_good = 0, g_cut = 0;

// cap_kind: 0: cap 0, 1: m - 1, 2: m, 3: m + 5; data_kind: 0: no data, 1: capacity 0, 2: inside the bytes, 3: the bytes, 4: above them
static int one(const Bytes& bytes, uint32_t k, uint32_t flags, const Bytes& dict_bytes, uint64_t bound, uint64_t base, uint32_t ss, uint32_t os, uint32_t ds, uint32_t ts,
               uint32_t item_elems, uint32_t cap_kind, uint32_t data_kind, bool has_offsets, bool backwards) {
  Block s(bytes.size(), ss);
  s.fill_random(rnd);
  for (size_t i = 0; i < bytes.size(); i++) s.at()[i] = bytes[i];
  Block t(dict_bytes.size(), ts);
  t.fill_random(rnd);
  for (size_t i = 0; i < dict_bytes.size(); i++) t.at()[i] = dict_bytes[i];
  const uint64_t count = expect(s.at(), s.len, k, flags, 0u).res.count;
  const uint64_t cap = cap_kind == 0u ? 0u : cap_kind == 1u ? (count ? count - 1u : 0u) : cap_kind == 2u ? count : count + 5u;
  const uint64_t m = count < cap ? count : cap;
  if (m > (1u << 20)) return 0;   // (seeded bytes may announce a run of a length nobody wants to see expanded here)
  const Want want = expect(s.at(), s.len, k, flags, m);
  // what the contract says of the column
  const Parsed dict = cap ? parse(t.at(), t.len, bound) : Parsed{{}, 0u, 0u};
  const uint64_t D = dict.entries.size();
  g_cut += dict.status;
  BrotliAmdUndictBytesResult must = brotli_amd_undict_bytes_result(want.res, BrotliAmdUndictBytesDictResult{D, dict.consumed, dict.status, 0u});
  std::vector<uint64_t> offs(1, base);
  Bytes body;
  for (size_t e = 0; e < want.idx.size(); e++) {
    if (want.idx[e] >= D) { must.bad++; if (e < must.first_bad) must.first_bad = e; }
    else body.insert(body.end(), dict.entries[want.idx[e]].begin(), dict.entries[want.idx[e]].end());
    offs.push_back(base + body.size());
  }
  must.bytes = body.size();
  g_bad += must.bad; g_good += want.idx.size() - must.bad;
  const uint64_t data_cap = data_kind <= 1u ? 0u : data_kind == 2u ? body.size() / 2u + (body.size() > 20u ? rnd() % 16u : 0u) : data_kind == 3u ? body.size() : body.size() + 9u;
  const uint64_t kept = data_kind == 0u ? 0u : body.size() < data_cap ? body.size() : data_cap;
  const uint32_t ow = brotli_amd_undict_bytes_offset_width(flags);
  const bool ends_only = (flags & BROTLI_AMD_UNDICT_BYTES_ENDS_ONLY) != 0u;
  const uint64_t slots = !has_offsets || cap == 0u ? 0u : m + (ends_only ? 0u : 1u);
  Block o((size_t)(slots * ow), os), d((size_t)kept, ds);
  o.fill_pattern();
  d.fill_pattern();
  // the phases
  const uint64_t nstarts = brotli_amd_undict_bytes_starts(t.len, bound);
  Block st(cap ? (size_t)(nstarts * 4u) : 0u, 0u);
  uint32_t* starts = reinterpret_cast<uint32_t*>(st.at());
  BrotliAmdUndictBytesDictResult dr = {0u, 0u, 0u, 0u};
  if (cap) dr = brotli_amd_undict_bytes_host_dict(t.addr(), t.len, bound, starts);
  const BrotliAmdUndictBytesSeg sg = {s.at(), data_kind ? d.at() : nullptr, s.len, cap, 0u, cap ? 0u : BROTLI_AMD_UNDICT_BYTES_NO_DICT,
                                      flags & BROTLI_AMD_UNDICT_BYTES_WIDTH_BYTE ? 0xEEu : k, flags, 0u, has_offsets ? o.at() : nullptr, data_cap, base};
  const uint64_t items = brotli_amd_unrle_items(cap < count + 1u ? cap : count + 1u, item_elems);
  BrotliAmdUndictBytesSeg walked = sg;
  walked.cap = cap < count + 1u ? cap : count + 1u;
  std::vector<BrotliAmdUnrleCheckpoint> ckpts((size_t)items, BrotliAmdUnrleCheckpoint{BROTLI_AMD_UNRLE_NONE, BROTLI_AMD_UNRLE_NONE});
  BrotliAmdUndictBytesResult got = brotli_amd_undict_bytes_host_walk(walked, dr, item_elems, ckpts.data());
  std::vector<BrotliAmdUndeltaTile> tiles((size_t)items);
  for (uint64_t i = 0; i < items; i++) { const uint64_t j = backwards ? items - 1u - i : i; tiles[(size_t)j] = brotli_amd_undict_bytes_host_count(walked, starts, &got, ckpts[(size_t)j], j, item_elems); }
  std::vector<uint64_t> carries((size_t)items);
  BrotliAmdUndeltaPair run = {0u, 0u};
  for (size_t j = 0; j < items; j++) {
    carries[j] = brotli_amd_undelta_carry_in(run.sum, tiles[j]);
    run = brotli_amd_undelta_combine(run, brotli_amd_undelta_tile_pair(tiles[j]));
  }
  std::vector<uint64_t> ends(item_elems + 1u);
  std::vector<uint32_t> pos(item_elems);
  for (uint64_t i = 0; i < items; i++) {
    const uint64_t j = backwards ? i : items - 1u - i;   // (the other way round than the counts)
    brotli_amd_undict_bytes_host_expand(walked, t.addr(), starts, &got, ckpts[(size_t)j], j, item_elems, carries[(size_t)j], ends.data(), pos.data(),
                                        [&](uint64_t words, auto each) { for (uint64_t q = 0; q < words; q++) each(backwards ? words - 1u - q : q); });
  }
  g_segments++;
  if (got.count != must.count || got.consumed != must.consumed || got.runs != must.runs || got.status != must.status || got.bits != must.bits || got.bad != must.bad ||
      got.first_bad != must.first_bad || got.bytes != must.bytes || got.dict_entries != must.dict_entries || got.dict_consumed != must.dict_consumed ||
      got.dict_status != must.dict_status) {
    std::fprintf(stderr, "k %u flags %u length %zu dictionary %zu bound %llu cap %llu: result %llu %llu %llu %u %u %llu %llu %llu %llu %llu %u, not %llu %llu %llu %u %u %llu %llu %llu %llu %llu %u\n",
                 k, flags, s.len, t.len, (unsigned long long)bound, (unsigned long long)cap, (unsigned long long)got.count, (unsigned long long)got.consumed,
                 (unsigned long long)got.runs, got.status, got.bits, (unsigned long long)got.bad, (unsigned long long)got.first_bad, (unsigned long long)got.bytes,
                 (unsigned long long)got.dict_entries, (unsigned long long)got.dict_consumed, got.dict_status, (unsigned long long)must.count, (unsigned long long)must.consumed,
                 (unsigned long long)must.runs, must.status, must.bits, (unsigned long long)must.bad, (unsigned long long)must.first_bad, (unsigned long long)must.bytes,
                 (unsigned long long)must.dict_entries, (unsigned long long)must.dict_consumed, must.dict_status);
    return 1;
  }
  size_t i = 0;
  uint8_t is = 0, should = 0;
  if (!o.holds([&](size_t p) { return (uint8_t)(offs[p / ow + (ends_only ? 1u : 0u)] >> (8u * (p % ow))); }, &i, &is, &should)) {
    std::fprintf(stderr, "k %u flags %u length %zu skews %u %u %u %u item %u: byte %zu of the offsets is %02x, not %02x\n", k, flags, s.len, ss, os, ds, ts, item_elems, i, is, should);
    return 1;
  }
  if (!d.holds([&](size_t p) { return body[p]; }, &i, &is, &should)) {
    std::fprintf(stderr, "k %u flags %u length %zu skews %u %u %u %u item %u data capacity %llu: byte %zu of the data is %02x, not %02x\n", k, flags, s.len, ss, os, ds, ts,
                 item_elems, (unsigned long long)data_cap, i, is, should);
    return 1;
  }
  return 0;
}

// a dictionary's entries for fields of k bits: none, one, a few, half of the indices, all of them
static uint64_t entries_for(uint32_t k, uint32_t pick) {
  const uint64_t all = (uint64_t)1 << (k < 9u ? k : 9u);
  switch (pick % 5u) {
    case 0u: return 0u;
    case 1u: return 1u;
    case 2u: return 3u + rnd() % 5u;
    case 3u: return all / 2u + 1u;
    default: return all;
  }
}
static uint32_t seeded_flags(uint32_t wb) {
  return wb | ((rnd() & 1u) ? BROTLI_AMD_UNDICT_BYTES_OFFSETS64 : 0u) | ((rnd() & 1u) ? BROTLI_AMD_UNDICT_BYTES_ENDS_ONLY : 0u);
}

int main() {
  const uint32_t item_sizes[4] = {8u, 24u, 40u, BROTLI_AMD_UNRLE_ITEM_ELEMS};
  const uint64_t all = BROTLI_AMD_UNDICT_BYTES_ALL;
  for (uint32_t k = 0; k <= 32u; k++) {
    for (uint32_t wb = 0; wb < 2u; wb++) {
      const Bytes whole = runs(k, 300u, wb != 0u);
      // whole, and cut; the dictionary whole, bounded, and cut at a seeded byte
      for (uint32_t r = 0; r < 15u; r++) {
        Bytes dict = dictionary(entries_for(k, r));
        const uint64_t bound = r % 3u == 1u ? entries_for(k, rnd()) : all;
        if (r % 4u == 3u && !dict.empty()) dict.resize(rnd() % dict.size());
        if (int e = one(whole, k, seeded_flags(wb), dict, bound, (rnd() & 1u) ? 0u : 0xFFFFFFF0u + rnd() % 32u, rnd() & 15u, rnd() & 15u, rnd() & 15u, rnd() & 15u, item_sizes[r & 3u],
                        r % 4u, r % 5u, r % 6u != 5u, (r & 4u) != 0u)) return e;
      }
      for (size_t cut = 0; cut < whole.size(); cut += cut < 24u ? 1u : 1u + rnd() % 60u)
        if (int e = one(Bytes(whole.begin(), whole.begin() + cut), k, seeded_flags(wb), dictionary(entries_for(k, rnd())), all, rnd() % 100u, rnd() & 15u, rnd() & 15u, rnd() & 15u,
                        rnd() & 15u, item_sizes[rnd() & 3u], 1u + rnd() % 3u, rnd() % 5u, true, (rnd() & 1u) != 0u)) return e;
    }
  }
  // every skew of the dictionary with every skew of the data, and every skew of the offsets
  for (uint32_t ts = 0; ts < 16u; ts++)
    for (uint32_t ds = 0; ds < 16u; ds++) {
      const uint32_t k = 1u + rnd() % 7u;
      if (int e = one(runs(k, 40u + rnd() % 100u, false), k, seeded_flags(0u), dictionary(((uint64_t)1 << k) - (ds & 1u)), all, 0u, rnd() & 15u, (ts + 3u * ds) & 15u, ds, ts,
                      item_sizes[(ts ^ ds) & 3u], 2u, 2u + (ds + ts) % 3u, true, (ts & 1u) != 0u)) return e;
    }
  // a dictionary cut at every byte
  {
    const Bytes dict = dictionary(6u), data = runs(3u, 60u, false);
    for (size_t cut = 0; cut <= dict.size(); cut++)
      if (int e = one(data, 3u, 0u, Bytes(dict.begin(), dict.begin() + cut), all, 0u, 1u, 2u, 3u, (uint32_t)cut & 15u, 8u, 2u, 3u, true, (cut & 1u) != 0u)) return e;
  }
  // far-out indices: RLE values of 0xFFFFFFFF and fields of 32 bits against a dictionary of three entries, and against none
  for (uint64_t D : {3u, 0u}) {
    Bytes b;
    put_header(&b, 6u << 1, 0u); for (int i = 0; i < 4; i++) b.push_back(0xFFu);
    put_header(&b, 1u << 1 | 1u, 0u); for (int i = 0; i < 32; i++) b.push_back((uint8_t)(i % 4 == 3 ? 0x80u | rnd() : rnd()));
    put_header(&b, 3u << 1, 0u); b.push_back(2u); b.push_back(0u); b.push_back(0u); b.push_back(0u);
    for (uint32_t ts = 0; ts < 16u; ts += 5u)
      if (int e = one(b, 32u, 0u, dictionary(D), all, 0u, 1u, 2u, 3u, ts, 8u, 2u, 3u, true, false)) return e;
  }
  // a width byte that is none, and no bytes at all
  if (int e = one(Bytes{33u, 0x10u, 0x05u}, 0u, 1u, dictionary(4u), all, 0u, 3u, 5u, 7u, 9u, 8u, 3u, 4u, true, false)) return e;
  if (int e = one(Bytes(), 3u, 1u, dictionary(4u), all, 7u, 0u, 0u, 0u, 0u, 8u, 3u, 4u, true, false)) return e;
  if (int e = one(Bytes(), 3u, 0u, Bytes(), all, 7u, 0u, 0u, 0u, 0u, 8u, 3u, 4u, true, false)) return e;
  if (g_bad == 0u || g_good == 0u || g_cut == 0u) { std::fprintf(stderr, "no bad index, no good index or no cut dictionary was seen\n"); return 1; }
  std::printf("%llu segments\n", g_segments);
  return 0;
}
