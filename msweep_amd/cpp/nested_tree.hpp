// nested_tree.hpp -- --nested of msweep_mini: the K >= 2 columns of -i as ONE hierarchy, column 0 the coarsest
// (DESIGN.md 7j).  A node is a list of group names (g0, ..., g(d-1)), the root the empty list; its stem is the names joined
// by `_`.  Here is everything about the tree that is judged before a device is touched, and the names of a node's files.
// msweep_amd/nested.py is the same for the Python driver, with the same messages.  Host code only:
// tests/cpp/nested_tree_test.cpp runs it stand alone.
#pragma once
#include <algorithm>
#include <cstddef>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

namespace msw_nested {

struct NestedError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

// the flags --nested refuses, in the order they are named when several are given
inline const std::vector<std::string> &conflicts() {
  static const std::vector<std::string> v = {"--read-likelihood", "--no-fit-model", "--alphas", "--write-unassigned",
                                             "--write-assignment-table", "--print-probs"};
  return v;
}

inline std::string stem(const std::vector<std::string> &names) {
  std::string s;
  for (size_t i = 0; i < names.size(); ++i) s += (i ? "_" : "") + names[i];
  return s;
}

// a label path as the messages print it
inline std::string show(const std::vector<std::string> &names) {
  if (names.empty()) return "(root)";
  std::string s;
  for (size_t i = 0; i < names.size(); ++i) s += (i ? " > " : "") + names[i];
  return s;
}

// a node's output: `<prefix>[_<stem>]_<name>` -- the root's names are the single-column names; without a prefix the bare
// name, `<stem>_<name>` below the root (the likelihood files: everything else goes to stdout then)
inline std::string node_path(const std::string &prefix, const std::string &node_stem, const std::string &name) {
  const std::string mid = node_stem.empty() ? std::string() : node_stem + "_";
  return prefix.empty() ? mid + name : prefix + "_" + mid + name;
}

// the file stem of a node's bin for `group`: `<group>` at the root, as without --nested, `<stem>_<group>` below
inline std::string bin_name(const std::string &node_stem, const std::string &group) {
  return node_stem.empty() ? group : node_stem + "_" + group;
}

// given: the flags of conflicts() that the command line holds
inline void check_flags(const std::vector<std::string> &given) {
  for (const std::string &flag : conflicts())
    if (std::find(given.begin(), given.end(), flag) != given.end()) throw NestedError("--nested can't be used with " + flag);
}

// rows: the fields of every line of the -i file (all of one length).  One column, a group name with '/', and two distinct
// label paths -- of any depth, the root included -- whose stems are the same name are refused: stems name the nodes' files
// and, one level down, the bins.
inline void check_tree(const std::string &path, const std::vector<std::vector<std::string>> &rows) {
  const size_t K = rows.empty() ? 0 : rows[0].size();
  if (K < 2) throw NestedError("--nested needs at least two columns in -i (" + path + " has " + std::to_string(K) + ")");
  std::map<std::string, std::vector<std::string>> seen;
  seen.emplace(std::string(), std::vector<std::string>());
  for (const auto &r : rows)
    for (size_t d = 1; d <= K; ++d) {
      const std::vector<std::string> p(r.begin(), r.begin() + d);
      if (p.back().find('/') != std::string::npos)
        throw NestedError(path + ": the group name " + p.back() + " contains '/' (--nested names files by group)");
      const std::string s = stem(p);
      const auto it = seen.emplace(s, p).first;
      if (it->second != p)
        throw NestedError(path + ": the label paths " + show(it->second) + " and " + show(p) + " give the same name `" + s + "`");
    }
}

}  // namespace msw_nested
