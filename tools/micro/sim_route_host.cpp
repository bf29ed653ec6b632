// Host driver of csrc/sim_route.h: what a similarity call would launch, without a GPU and without HIP.  The switches come
// from the environment (sim_switches_from_env, as in the library); every line of stdin is one case of key=value words,
//   f=384 nvox=8640 half=1 mode=0 feat=256 ws=1 cus=256 counts=70,3,33   classes=3 n2=18 o0=24 o1=20 o2=36 sim=256 out=256
// (feat, sim, out: addresses, only their alignment is read; ws: a large-enough matrix-core workspace was given; the second
// group describes the quantise launch, `classes` there defaults to the number of counts), and every case prints one JSON line:
// the accumulation form and name, the quantise form and shift, and the chunk plan of the VALU kernels for these counts.
//
//   c++ -std=c++17 -O1 tools/micro/sim_route_host.cpp -o tools/micro/sim_route_host
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/micro/sim_route_host.cpp
//       -o tools/micro/sim_route_host        (by hand, on a CPU machine; tests/test_sim_route_cpu.py builds the plain one)
#include <cstdio>
#include <cstring>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../../vit-tf_amd/csrc/sim_route.h"

static void print_ints(const char* key, const int* v, int n) {
  std::printf("\"%s\": [", key);
  for (int i = 0; i < n; ++i) std::printf("%s%d", i ? ", " : "", v[i]);
  std::printf("]");
}

int main() {
  static const char* const accum_names[] = {"few", "f768", "two_blocks", "dma", "strided", "valu_split", "valu"};
  static const char* const quant_names[] = {"bytes", "16", "pow2"};
  const SimSwitches sw = sim_switches_from_env();
  char line[1 << 16];
  while (std::fgets(line, sizeof line, stdin)) {
    std::map<std::string, long long> arg = {{"f", 384}, {"nvox", 4096}, {"half", 1}, {"mode", 0}, {"feat", 256}, {"ws", 1}, {"cus", 256},
                                            {"classes", 0}, {"n2", 16}, {"o0", 16}, {"o1", 16}, {"o2", 16}, {"sim", 256}, {"out", 256}};
    std::vector<int32_t> start = {0};
    std::istringstream words(line);
    std::string word;
    while (words >> word) {
      const size_t eq = word.find('=');
      if (eq == std::string::npos) { std::fprintf(stderr, "not key=value: %s\n", word.c_str()); return 2; }
      const std::string key = word.substr(0, eq), value = word.substr(eq + 1);
      if (key == "counts") {
        std::istringstream list(value);
        std::string n;
        while (std::getline(list, n, ',')) start.push_back(start.back() + std::stoi(n));
      } else if (arg.count(key)) {
        arg[key] = std::stoll(value);
      } else {
        std::fprintf(stderr, "unknown key: %s\n", key.c_str());
        return 2;
      }
    }
    const int classes = (int)start.size() - 1;
    if (classes < 1) continue;                                 // (an empty line)
    const SimRoute r = sim_route_accumulate((int)arg["f"], arg["nvox"], start.data(), classes, arg["half"] != 0, (int)arg["mode"],
                                            (uintptr_t)arg["feat"], arg["ws"] != 0, (int)arg["cus"], sw);
    const SimQuantRoute q = sim_route_quantize(arg["classes"] ? (int)arg["classes"] : classes, (int)arg["n2"], (int)arg["o0"], (int)arg["o1"],
                                               (int)arg["o2"], (uintptr_t)arg["sim"], (uintptr_t)arg["out"], sw);
    std::printf("{\"accumulate\": {\"form\": \"%s\", \"name\": \"%s\"}, \"quantize\": {\"form\": \"%s\", \"shift\": %d}, \"chunks\": [",
                accum_names[r.form], r.name, quant_names[q.form], q.shift);
    for (int a0 = 0; a0 < start[classes];) {
      SimChunk ch;
      std::memset(&ch, 0x5a, sizeof ch);                       // (every field the kernels read must be written by the walk)
      const int n = sim_next_chunk(start.data(), classes, a0, &ch);
      std::printf("%s{\"a0\": %d, \"n\": %d, \"n_ann\": %d, \"c0\": %d, \"nc\": %d, ", a0 ? ", " : "", a0, n, ch.n_ann, ch.c0, ch.nc);
      print_ints("cls", ch.cls, ACH);
      std::printf(", ");
      print_ints("first", ch.first, MAXC);
      std::printf(", ");
      print_ints("last", ch.last, MAXC);
      std::printf(", \"count\": [");
      for (int i = 0; i < MAXC; ++i) std::printf("%s%g", i ? ", " : "", (double)ch.count[i]);
      std::printf("]}");
      if (n < 1) return 1;                                     // (the walk must advance)
      a0 += n;
    }
    std::printf("]}\n");
  }
  return 0;
}
