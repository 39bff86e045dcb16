// samples_manifest.hpp -- --samples FILE of msweep_mini: the manifest of a study, one sample per line,
// `<prefix> TAB <alignment files> [TAB <FASTQ files>]` with comma separated lists, everything about it that is judged
// before a device is touched, and the queue the workers take their samples from.  Empty lines and lines
// beginning with `#` are skipped.  msweep_amd/samples.py is the same parser with the same messages for the Python driver.
// Host code only: tests/cpp/samples_manifest_test.cpp runs it stand alone under the sanitizers.
#pragma once
#include <cstddef>
#include <fstream>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

namespace msw_samples {

struct ManifestError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

struct Sample {
  std::string prefix;
  std::vector<std::string> files, fastqs;
  bool have_fastqs = false;  // a third column
  size_t line = 0;
};

// the command line's own flags for what a manifest line gives, in the order they are named when they collide
inline const std::vector<std::string> &conflicts() {
  static const std::vector<std::string> v = {"--themisto", "--themisto-1", "--themisto-2", "-o", "--read-likelihood", "--print-probs",
                                             "--extract-reads"};
  return v;
}

// every element counts, an empty one too
inline std::vector<std::string> split_all(const std::string &s, char d) {
  std::vector<std::string> out;
  for (size_t b = 0;;) {
    const size_t e = s.find(d, b);
    out.push_back(s.substr(b, e == std::string::npos ? e : e - b));
    if (e == std::string::npos) break;
    b = e + 1;
  }
  return out;
}

// `p` without empty and `.` components, `..` resolved against the component before it: two spellings of one place
// compare equal (no look at the file system: the directories may not exist yet)
inline std::string normal_path(const std::string &p) {
  const bool abs = !p.empty() && p[0] == '/';
  std::vector<std::string> parts;
  for (const std::string &c : split_all(p, '/')) {
    if (c.empty() || c == ".") continue;
    if (c == ".." && !parts.empty() && parts.back() != "..") parts.pop_back();
    else if (c == ".." && abs) continue;
    else parts.push_back(c);
  }
  std::string out = abs ? "/" : "";
  for (size_t i = 0; i < parts.size(); ++i) out += (i ? "/" : "") + parts[i];
  return out;
}

// where a sample's bins and extracted reads go (bin_path): the prefix up to its last '/', or '.'
inline std::string bin_dir(const std::string &prefix) {
  const size_t s = prefix.rfind('/');
  return normal_path(s == std::string::npos ? std::string(".") : prefix.substr(0, s) + "/");
}

// the samples of the manifest, in its order
inline std::vector<Sample> read_manifest(const std::string &path) {
  std::ifstream in(path, std::ios::binary);
  if (!in) throw ManifestError("cannot open the sample manifest " + path);
  std::vector<Sample> out;
  std::string line;
  size_t n = 0;
  while (std::getline(in, line)) {
    ++n;
    if (!line.empty() && line.back() == '\r') line.pop_back();
    if (line.empty() || line[0] == '#') continue;
    const std::vector<std::string> cols = split_all(line, '\t');
    const std::string where = path + ", line " + std::to_string(n) + ": ";
    if (cols.size() < 2 || cols.size() > 3)
      throw ManifestError(where + std::to_string(cols.size()) + " columns (a sample is <prefix> TAB <alignment files> [TAB <FASTQ files>])");
    if (cols[0].empty()) throw ManifestError(where + "empty output prefix");
    Sample s;
    s.prefix = cols[0];
    s.files = split_all(cols[1], ',');
    s.have_fastqs = cols.size() == 3;
    if (s.have_fastqs) s.fastqs = split_all(cols[2], ',');
    for (const auto *l : {&s.files, &s.fastqs})
      for (const std::string &p : *l)
        if (p.empty()) throw ManifestError(where + "empty path in a list");
    s.line = n;
    out.push_back(std::move(s));
  }
  if (out.empty()) throw ManifestError("the sample manifest " + path + " has no sample");
  return out;
}

// what makes two samples of one run collide, and the third column's conditions
inline void check_samples(const std::string &path, const std::vector<Sample> &samples, bool bin_reads) {
  auto where = [&](const Sample &s) { return path + ", line " + std::to_string(s.line) + ": "; };
  for (const Sample &s : samples)
    if (s.have_fastqs != samples[0].have_fastqs) throw ManifestError(where(s) + "FASTQ files on some lines and not on others");
  if (samples[0].have_fastqs && !bin_reads) throw ManifestError(path + ": a FASTQ column needs --bin-reads");
  std::map<std::string, size_t> prefixes, dirs;
  for (const Sample &s : samples) {
    const auto ins = prefixes.emplace(normal_path(s.prefix), s.line);
    if (!ins.second)
      throw ManifestError(where(s) + "the output prefix " + s.prefix + " is that of line " + std::to_string(ins.first->second));
  }
  if (!bin_reads) return;
  // the bins <dir>/<group>.bin and the extracted reads carry no prefix
  for (const Sample &s : samples) {
    const auto ins = dirs.emplace(bin_dir(s.prefix), s.line);
    if (!ins.second)
      throw ManifestError(where(s) + "with --bin-reads the prefix " + s.prefix + " lies in the directory of line " +
                          std::to_string(ins.first->second) + ": the bins would overwrite each other");
  }
}

// --devices d0[,d1,...]: one worker per entry, an entry may repeat
inline std::vector<int> parse_devices(const std::string &text) {
  std::vector<int> devs;
  for (const std::string &x : split_all(text, ',')) {
    if (x.empty() || x.size() > 9 || x.find_first_not_of("0123456789") != std::string::npos)
      throw ManifestError("--devices: " + text + " is not a list of device indices");
    devs.push_back(std::stoi(x));
  }
  return devs;
}

// The refusals of --samples / --devices in their order.  `given`: the flags of conflicts() that the command line holds.
inline std::vector<Sample> from_args(const std::vector<std::string> &given, bool have_samples, const std::string &samples_path,
                                     bool have_devices, const std::string &devices, bool bin_reads, std::vector<int> &devs_out) {
  if (!have_samples) throw ManifestError("--devices needs --samples");
  for (const std::string &flag : conflicts())
    for (const std::string &g : given)
      if (g == flag) throw ManifestError("--samples can't be used with " + flag);
  devs_out.clear();
  if (have_devices) devs_out = parse_devices(devices);
  std::vector<Sample> samples = read_manifest(samples_path);
  check_samples(samples_path, samples, bin_reads);
  return samples;
}

// The workers' queue: samples are handed out in manifest order; after the first failure none is started any more (those in
// flight finish).
class Queue {
 public:
  explicit Queue(size_t n) : n_(n) {}
  // the index of the next sample to run; false: nothing more to start
  bool next(size_t &index) {
    std::lock_guard<std::mutex> g(mu_);
    if (failed_ || next_ >= n_) return false;
    index = next_++;
    return true;
  }
  void done(bool ok) {
    std::lock_guard<std::mutex> g(mu_);
    ++(ok ? finished_ : failed_);
  }
  size_t finished() const { return finished_; }
  size_t failed() const { return failed_; }
  size_t not_started() const { return n_ - finished_ - failed_; }  // (once the workers have joined)

 private:
  std::mutex mu_;
  size_t n_, next_ = 0, finished_ = 0, failed_ = 0;
};

}  // namespace msw_samples
