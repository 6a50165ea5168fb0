// Driver of tests/test_topic_summaries_model.py: the C++ writer of TopWords.txt / RelevanceWords.txt (include/ggs_formats.hpp)
// on the rows the test sends.  usage: driver <file>; stdin: one topic per line, its words separated by blanks.
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "ggs_formats.hpp"

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  std::vector<std::vector<std::string>> rows;
  std::string line;
  while (std::getline(std::cin, line)) {
    rows.emplace_back();
    std::istringstream in(line);
    std::string w;
    while (in >> w) rows.back().push_back(w);
  }
  ggs::formats::write_top_words(rows, argv[1]);
  return 0;
}
