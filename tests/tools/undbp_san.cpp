// undbp_san.cpp -- the undbp varint, header, block, group and item functions (csrc/brotli_undbp.h) under AddressSanitizer and UBSan, as a
// program of its own:
//   g++ -std=c++17 -fsanitize=address,undefined -I include -I rust-brotli-decompressor_amd/csrc tests/tools/undbp_san.cpp
// The walk, the items' sums, the carries and the items' stores, with items of 32, 64 and 96 deltas and the device's own, forwards or backwards,
// against a serial decoder of its own.  Streams of seeded values with B and M of (128, 1), (128, 4), (256, 4), (1024, 8) and (1024, 32),
// widths of 0 .. 64 bits, varints padded to seeded lengths and junk in the unneeded width bytes; whole, cut at every length up to 64 bytes and
// at seeded lengths beyond, and with seeded bytes in seeded places (which stop the decode in every way there is); segments of nothing but seeded
// bytes; capacities of 0, m - 1, m and m + 5; every pair of skews for short ones.  Every source lies in a heap block of EXACTLY the
// sixteen-byte words its span touches, every destination in one of the words its min(m, cap) elements touch: a load or a store one word too
// far would be reported; the destination's bytes beside the elements must keep their pattern.  Exits 0 when everything agreed.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "brotli_device_abi.h"
#include "brotli_undbp.h"
#include "san_block.h"

static uint32_t g_seed = 2031u;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }
static uint64_t rnd64() { return ((uint64_t)rnd() << 48) ^ ((uint64_t)rnd() << 24) ^ rnd(); }

typedef SanBlock Block;
typedef std::vector<uint8_t> Bytes;

struct Want { std::vector<uint64_t> elems; BrotliAmdUndbpResult res; };

// a varint one byte after the other: 0 and *value, *bytes; or the status
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

// the contract of include/brotli/batch.h, one field after the other; at most `keep` elements are kept
static Want expect(const uint8_t* s, size_t len, uint64_t keep) {
  Want out;
  out.res = BrotliAmdUndbpResult{0u, 0u, 0u, 0u, BROTLI_AMD_UNDBP_OK, 0u, 0u};
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
  out.res.consumed = off;
  if (N == 0u) return out;
  const uint64_t V = B / M;
  uint64_t v = unzigzag(h[3]), count = 1;
  if (keep) out.elems.push_back(v);
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
        if (out.elems.size() < keep) out.elems.push_back(v);
      }
      got += want;
      pos = out.res.status == BROTLI_AMD_UNDBP_OK ? pos + (size_t)bytes : len;
    }
    if (got) out.res.blocks++;
    count += got; off = pos;
    if (out.res.status != BROTLI_AMD_UNDBP_OK) break;
  }
  out.res.count = count; out.res.consumed = off;
  return out;
}

static void put_varint(Bytes* out, uint64_t v, uint32_t pad) {
  Bytes b;
  do { b.push_back((uint8_t)(v & 0x7Fu)); v >>= 7; } while (v);
  while (b.size() < pad && b.size() < 10u) b.push_back(0u);
  for (size_t i = 0; i + 1u < b.size(); i++) b[i] |= 0x80u;
  out->insert(out->end(), b.begin(), b.end());
}
static uint32_t pad() { return (rnd() % 4u) ? 0u : 1u + rnd() % 10u; }

// a stream of n values whose fields have seeded widths up to max_bits
static Bytes stream(uint32_t B, uint32_t M, uint32_t n, uint32_t max_bits) {
  Bytes out;
  const uint32_t V = B / M;
  put_varint(&out, B, pad()); put_varint(&out, M, pad()); put_varint(&out, n, pad()); put_varint(&out, rnd64(), pad());
  for (uint32_t left = n ? n - 1u : 0u; left != 0u;) {
    put_varint(&out, (rnd() & 1u) ? rnd64() : rnd() % 9u, pad());
    const uint32_t need = (left < B ? left : B), minis = (need + V - 1u) / V;
    Bytes widths;
    for (uint32_t j = 0; j < M; j++) widths.push_back(j < minis ? (uint8_t)(rnd() % (max_bits + 1u)) : (uint8_t)rnd());
    out.insert(out.end(), widths.begin(), widths.end());
    for (uint32_t j = 0; j < minis; j++)
      for (uint32_t i = 0; i < V / 8u * widths[j]; i++) out.push_back((uint8_t)rnd());
    left -= need;
  }
  return out;
}

static unsigned long long g_segments = 0;

// cap_kind: 0: cap 0, 1: m - 1, 2: m, 3: m + 5
static int one(const Bytes& bytes, uint32_t w, uint32_t ss, uint32_t ds, uint32_t item_deltas, uint32_t cap_kind, bool backwards) {
  Block s(bytes.size(), ss);
  s.fill_random(rnd);
  for (size_t i = 0; i < bytes.size(); i++) s.at()[i] = bytes[i];
  const uint64_t m = expect(s.at(), s.len, 0u).res.count;
  const uint64_t cap = cap_kind == 0u ? 0u : cap_kind == 1u ? (m ? m - 1u : 0u) : cap_kind == 2u ? m : m + 5u;
  const uint64_t kept = m < cap ? m : cap;
  const Want want = expect(s.at(), s.len, kept);
  Block d((size_t)(kept * w), ds);
  d.fill_pattern();
  const BrotliAmdUndbpSeg sg = {s.at(), d.at(), s.len, cap, 0u, w, 0u};
  const uint64_t items = brotli_amd_undbp_items(cap, item_deltas);
  std::vector<BrotliAmdUndbpCheckpoint> ckpts((size_t)items, BrotliAmdUndbpCheckpoint{BROTLI_AMD_UNDBP_NONE, BROTLI_AMD_UNDBP_NONE});
  uint64_t first = 0;
  const BrotliAmdUndbpResult got = brotli_amd_undbp_host_walk(sg, item_deltas, ckpts.data(), &first);
  std::vector<BrotliAmdUndeltaTile> tiles((size_t)items);
  std::vector<uint64_t> carries((size_t)items);
  for (uint64_t i = 0; i < items; i++) { const uint64_t j = backwards ? items - 1u - i : i; tiles[(size_t)j] = brotli_amd_undbp_host_sum(sg, got, ckpts[(size_t)j], first, j, item_deltas); }
  BrotliAmdUndeltaPair run = {0u, 0u};
  for (uint64_t j = 0; j < items; j++) {
    carries[(size_t)j] = brotli_amd_undelta_carry_in(run.sum, tiles[(size_t)j]);
    run = brotli_amd_undelta_combine(run, brotli_amd_undelta_tile_pair(tiles[(size_t)j]));
  }
  for (uint64_t i = 0; i < items; i++) { const uint64_t j = backwards ? i : items - 1u - i; brotli_amd_undbp_host_store(sg, got, ckpts[(size_t)j], first, j, item_deltas, carries[(size_t)j]); }
  g_segments++;
  if (got.count != want.res.count || got.consumed != want.res.consumed || got.declared != want.res.declared || got.blocks != want.res.blocks ||
      got.status != want.res.status || got.block_values != want.res.block_values || got.miniblocks != want.res.miniblocks) {
    std::fprintf(stderr, "width %u length %zu skews %u %u: result %llu %llu %llu %llu %u %u %u, not %llu %llu %llu %llu %u %u %u\n", w, s.len, ss, ds,
                 (unsigned long long)got.count, (unsigned long long)got.consumed, (unsigned long long)got.declared, (unsigned long long)got.blocks, got.status,
                 got.block_values, got.miniblocks, (unsigned long long)want.res.count, (unsigned long long)want.res.consumed, (unsigned long long)want.res.declared,
                 (unsigned long long)want.res.blocks, want.res.status, want.res.block_values, want.res.miniblocks);
    return 1;
  }
  size_t i = 0;
  uint8_t is = 0, must = 0;
  if (d.holds([&](size_t p) { return (uint8_t)(want.elems[p / w] >> (8u * (p % w))); }, &i, &is, &must)) return 0;
  std::fprintf(stderr, "width %u length %zu skews %u %u item %u: byte %zu is %02x, not %02x\n", w, s.len, ss, ds, item_deltas, i, is, must);
  return 1;
}

int main() {
  const uint32_t item_sizes[4] = {32u, 64u, 96u, BROTLI_AMD_UNDBP_ITEM_DELTAS};
  const uint32_t shapes[5][2] = {{128u, 1u}, {128u, 4u}, {256u, 4u}, {1024u, 8u}, {1024u, 32u}};
  for (const auto& shape : shapes) {
    const uint32_t B = shape[0], M = shape[1];
    for (uint32_t max_bits : {0u, 3u, 12u, 33u, 64u}) {
      for (uint32_t w : {1u, 2u, 4u, 8u}) {
        const Bytes whole = stream(B, M, 2u * B + B / M + 1u + rnd() % 40u, max_bits);
        // whole, and cut
        for (uint32_t r = 0; r < 8u; r++)
          if (int e = one(whole, w, rnd() & 15u, rnd() & 15u, item_sizes[r & 3u], r & 3u, (r & 4u) != 0u)) return e;
        for (size_t cut = 0; cut < whole.size(); cut += cut < 64u ? 1u : 1u + rnd() % (whole.size() / 24u + 1u))
          if (int e = one(Bytes(whole.begin(), whole.begin() + cut), w, rnd() & 15u, rnd() & 15u, item_sizes[rnd() & 3u], rnd() & 3u, (rnd() & 1u) != 0u)) return e;
        // seeded bytes in seeded places of a short stream, and alone
        for (uint32_t r = 0; r < 16u; r++) {
          Bytes b = r < 12u ? stream(B, M, 1u + rnd() % (B + 40u), max_bits) : Bytes();
          if (r < 12u) for (uint32_t i = 0, n = 1u + rnd() % 3u; i < n; i++) b[rnd() % (b.size() < 40u ? b.size() : 40u)] = (uint8_t)((rnd() & 1u) ? rnd() : 0x80u | rnd());
          else for (uint32_t i = 0, n = rnd() % 30u; i < n; i++) b.push_back((uint8_t)((rnd() & 3u) ? rnd() : 0x80u | rnd()));
          // (seeded bytes may declare more values than anybody wants to see here: the stream is short, so they do not get far)
          if (int e = one(b, w, rnd() & 15u, rnd() & 15u, item_sizes[rnd() & 3u], 2u + (rnd() & 1u), (rnd() & 1u) != 0u)) return e;
        }
      }
    }
  }
  // every pair of skews
  for (uint32_t ss = 0; ss < 16u; ss++)
    for (uint32_t ds = 0; ds < 16u; ds++) {
      const uint32_t w = 1u << ((ss + ds) & 3u);
      if (int e = one(stream(128u, 4u, 1u + rnd() % 300u, 1u + rnd() % 64u), w, ss, ds, item_sizes[(ss ^ ds) & 3u], 1u + (ds & 1u) * 2u, (ss & 1u) != 0u)) return e;
    }
  // no bytes at all
  for (uint32_t w : {1u, 2u, 4u, 8u})
    if (int e = one(Bytes(), w, 0u, 0u, 32u, 3u, false)) return e;
  std::printf("%llu segments\n", g_segments);
  return 0;
}
