// Driver of tests/test_min_distances_model.py: the C++ writers of min_doc_distances.csv and min_topic_distances.csv
// (include/ggs_formats.hpp) on the values the test sends.  usage: driver <log_dir>; stdin: one record per line,
//   D <iteration> <n> <bits of value 0, hex> ... <bits of value n-1>      -> append_min_doc_distances
//   T <iteration> <bits of the value, hex>                                 -> append_min_topic_distance
#include <cstdint>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "ggs_formats.hpp"

static double from_bits(const std::string &hex) {
  const uint64_t b = std::stoull(hex, nullptr, 16);
  double d;
  std::memcpy(&d, &b, 8);
  return d;
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  std::string kind;
  while (std::cin >> kind) {
    int iteration = 0;
    std::cin >> iteration;
    if (kind == "D") {
      long long n = 0;
      std::cin >> n;
      std::vector<double> v((size_t)n);
      for (auto &x : v) { std::string hex; std::cin >> hex; x = from_bits(hex); }
      ggs::formats::append_min_doc_distances(argv[1], iteration, v.data(), n);
    } else if (kind == "T") {
      std::string hex;
      std::cin >> hex;
      ggs::formats::append_min_topic_distance(argv[1], iteration, from_bits(hex));
    } else {
      return 3;
    }
  }
  return 0;
}
