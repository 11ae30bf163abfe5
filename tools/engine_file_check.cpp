// engine_file_check -- what the library's engine-file parser (csrc/engine_file.h) answers for a file, as a program of its own: nothing of
// libspvo.so is linked, so it builds with the host compiler and runs under the sanitizers (tests/test_engine_file_cpu.py):
//   g++ -std=c++17 -fsanitize=address,undefined tools/engine_file_check.cpp -o engine_file_check
//   engine_file_check FILE NET_HEIGHT   ->   "<status> <text>", or "0 <tensors> <ops> <payload floats> <precision>" for a file it accepts
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../superpoint-stereo-visual-odometry_amd/csrc/engine_file.h"

int main(int argc, char **argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s FILE NET_HEIGHT\n", argv[0]);
    return 2;
  }
  FILE *fh = std::fopen(argv[1], "rb");
  if (!fh) {
    std::printf("%d no such engine file: %s\n", SPVO_ERR_IO, argv[1]);
    return 0;
  }
  std::vector<unsigned char> buf;
  unsigned char chunk[65536];
  for (size_t n; (n = std::fread(chunk, 1, sizeof chunk, fh)) > 0;) buf.insert(buf.end(), chunk, chunk + n);
  std::fclose(fh);
  // an exact-size copy: a read one byte past the file's end is a read past the allocation, which the address sanitizer reports
  std::vector<unsigned char> exact(buf.begin(), buf.end());
  exact.shrink_to_fit();
  const spvo_int::EngineFile f = spvo_int::parse_engine_file(exact.data(), exact.size(), std::atoi(argv[2]), argv[1]);
  if (f.status) {
    std::printf("%d %s\n", f.status, f.error.c_str());
    return 0;
  }
  double sum = 0;   // every record and every float of the payload the parser vouches for is readable
  for (const auto &t : f.tensors) sum += t.ch + t.level;
  for (const auto &o : f.ops) sum += o.v[0] + (double)o.w_off;
  for (uint64_t i = 0; i < f.n_payload; ++i) sum += f.payload[i];
  std::printf("0 %zu %zu %llu %u%s\n", f.tensors.size(), f.ops.size(), (unsigned long long)f.n_payload, f.precision, sum == sum ? "" : " (payload holds NaN)");
  return 0;
}
