// Driver of tests/test_topic_diagnostics_model.py: the C++ writer of the topic-diagnostics CSV (include/ggs_formats.hpp) on the
// columns the test sends.  usage: driver <file>; stdin: the names on the first line, then one column per line, its doubles as
// hexadecimal floats (or nan / inf / -inf), all separated by blanks.
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "ggs_formats.hpp"

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  std::vector<std::string> names;
  std::vector<std::vector<double>> columns;
  std::string line, w;
  if (!std::getline(std::cin, line)) return 2;
  {
    std::istringstream in(line);
    while (in >> w) names.push_back(w);
  }
  while (std::getline(std::cin, line)) {
    columns.emplace_back();
    std::istringstream in(line);
    while (in >> w) columns.back().push_back(std::strtod(w.c_str(), nullptr));
  }
  ggs::formats::write_topic_diagnostics(names, columns, argv[1]);
  return 0;
}
