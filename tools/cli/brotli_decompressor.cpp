// brotli-decompressor [-dict=FILE] [--] [in [out]] -- the reference's command-line tool (src/bin/brotli-decompressor.rs:325-359) on top
// of include/brotli/reader.hpp: stdin/stdout by default, 64 KiB buffers, "Invalid Data"/"Unexpected EOF" on stderr.
// -dict=FILE: the stream was made for a custom (LZ77 prefix) dictionary, the file's bytes (at most 50331660 of them, as in the reference).
#include <cstdio>
#include <cstring>
#include <vector>

#include "brotli/reader.hpp"

namespace {
struct FileSource {
  FILE* f;
  size_t read(uint8_t* dst, size_t n) { return fread(dst, 1, n, f); }
};
}  // namespace

int main(int argc, char** argv) {
  FILE* in = stdin;
  FILE* out = stdout;
  std::vector<uint8_t> dictionary;
  bool double_dash = false;
  int files = 0;
  for (int a = 1; a < argc; a++) {
    if (!double_dash && std::strcmp(argv[a], "--") == 0) { double_dash = true; continue; }
    if (!double_dash && std::strncmp(argv[a], "-dict=", 6) == 0) {
      FILE* df = std::fopen(argv[a] + 6, "rb");
      if (!df) { std::perror(argv[a] + 6); return 1; }
      uint8_t piece[65536];
      for (size_t n; (n = std::fread(piece, 1, sizeof piece, df)) != 0;) dictionary.insert(dictionary.end(), piece, piece + n);
      std::fclose(df);
      if (dictionary.size() > 50331660u) { std::fprintf(stderr, "Dictionary larger than 50331660\n"); return 1; }
      continue;
    }
    if (files == 0) { if (!(in = std::fopen(argv[a], "rb"))) { std::perror(argv[a]); return 1; } }
    else if (files == 1) { if (!(out = std::fopen(argv[a], "wb"))) { std::perror(argv[a]); return 1; } }
    else { std::fprintf(stderr, "Cannot specify more than 2 filename args (input, output)\n"); return 1; }
    files++;
  }
  try {
    brotli_amd::Decompressor<FileSource> r(FileSource{in}, 65536, dictionary);
    std::vector<uint8_t> buf(65536);
    for (;;) {
      size_t n = r.read(buf.data(), buf.size());
      if (n == 0) break;
      if (std::fwrite(buf.data(), 1, n, out) != n) { std::perror("write"); return 1; }
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  if (out != stdout) std::fclose(out);
  return 0;
}
