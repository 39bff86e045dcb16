// msweep_mini.cpp -- the estimation path of mSWEEP's main() (src/mSWEEP.cpp:258-551) as a native
// host program over the C ABI: group indicators (-i, include/Reference.hpp / Grouping.hpp), Themisto
// plaintext pseudoalignments (the reader on the device: msw_alignment_read_device), likelihood built and kept on the
// GPU (msw_core_build_likelihood), RCG / EM abundances (--algorithm rcggpu|emgpu), bootstrap
// (--iters / --seed / --bootstrap-count, src/mSWEEP.cpp:496-518) and abundances.txt in the format of
// PlainSample / BootstrapSample::write_abundances[2] (src/PlainSample.cpp:32-71,
// src/BootstrapSample.cpp:75-130), plus the consumers around the path: --write-probs / --print-probs (Sample::write_probs,
// src/Sample.cpp:63-85,154-186: streamed from the device in blocks of ECs), --write-likelihood / --read-likelihood /
// --write-likelihood-bitseq / --no-fit-model (include/Likelihood.hpp:224-311, src/mSWEEP.cpp:357-386; the text of these
// matrices is formatted on the device, msw_core_text_block, and only its bytes come to the host), --run-rate (src/Sample.cpp:99-152,
// src/mSWEEP.cpp:524-548) and --bin-reads / --target-groups / --min-abundance (the mGEMS bins, src/mSWEEP.cpp:437-469:
// the bin pass on the device, msw_core_bin_reads_aln; the driver's choices are those of msweep_amd/binning.py), and
// --compress z / --compression-level (src/mSWEEP.cpp:107-109, src/OutfileDesignator.cpp:30-62: the matrix outputs and the
// bins as `<name>.gz`, the gzip stream compressed on the device, msw_core_gzip_*; bz2, lzma and zstd are refused).  Same flags and messages as the reference for what it covers; held byte-for-byte against
// the Python mirror `python -m msweep_amd` in tests/test_gpu_cli_toy.py.
// --extract-reads A[,B,...] (with --bin-reads): `<dir>/<group>_<k>.fastq[.gz]`, the binned reads of the k-th FASTQ file
// themselves, gathered on the device where the file lies (msw_fastq_*; the step docs/pipeline.md:59-64 gives to mGEMS).
// --write-unassigned / --write-assignment-table (with --bin-reads): `<dir>/unassigned_reads.bin`, the aligned reads no
// estimated group claims, and `<prefix>_reads_to_groups.tsv`, a 0/1 column per target for every aligned read, formatted on
// the device (msw_core_assign_reads_aln, msw_core_assign_table_block).
// --write-read-probs / --probs-threshold x: `<prefix>_read_probs.tsv`, one line `read id, group, probability` per aligned
// read and group at or above x, selected and formatted on the device (msw_core_sparse_probs_*; DESIGN.md 7k;
// tests/test_gpu_cli_read_probs.py).
// Every tab-separated column of the -i file is a grouping of its own and the whole estimation runs once per column
// (src/mSWEEP.cpp:282) -- from ONE read of the pseudoalignment, whose classes stay in device memory: run_grouping() is the
// body of that loop, out_path() names its files (`<prefix>_<i>_...` when there are several; tests/test_gpu_groupings.py).
// --samples FILE runs a whole manifest of samples (samples_manifest.hpp) in this one process: -i is read once, every worker
// (--devices, one std::thread per entry) keeps one handle for its life and takes the next sample from a shared queue, and
// each sample's files are those a single run with its -o / --themisto / --extract-reads writes (run_samples).
// --nested makes the K >= 2 columns of -i ONE hierarchy, column 0 the coarsest: every node of the tree runs run_grouping(),
// and every bin of a node is estimated within its group from a sub-alignment made on the device (msw_alignment_subset;
// run_nested_node, nested_tree.hpp); files `<prefix>_<stem>_...` (tests/test_gpu_cli_nested.py).
//
//   g++ -std=c++17 -O2 -o msweep_mini msweep_mini.cpp -L.. -lmsweep_core -Wl,-rpath,..
#include <algorithm>
#include <cerrno>
#include <charconv>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>
#include <map>
#include <mutex>
#include <random>
#include <sstream>
#include <stdexcept>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/msweep_core.h"
#include "nested_tree.hpp"
#include "samples_manifest.hpp"

namespace {

const char *kVersion = "msweep-amd-0.1.0";

struct Args {
  std::vector<std::string> themisto;
  std::string mode = "intersection", indicators, prefix, algorithm = "rcgcpu", emprecision = "double", alphas;
  size_t iters = 0, seed = 26012023, bootstrap_count = 0, min_hits = 0, max_iters = 5000;
  double q = 0.65, e = 0.01, zero_inflation = 0.01, tol = 1e-6;
  int gpu = 0;
  bool verbose = false;
  bool write_probs = false, print_probs = false, write_likelihood = false, no_fit_model = false, run_rate = false;
  bool write_likelihood_bitseq = false;
  std::string read_likelihood;
  bool bin_reads = false, have_target_groups = false, have_min_abundance = false;
  std::vector<std::string> target_groups;
  double min_abundance = 0.0;
  bool write_unassigned = false, write_assignment_table = false;  // with --bin-reads: the unassigned bin, the table
  // --write-read-probs / --probs-threshold x: <prefix>_read_probs.tsv, the probabilities at or above x per aligned read
  bool write_read_probs = false, have_probs_threshold = false;
  std::string probs_threshold;
  double probs_tau = 0.001;
  bool have_extract_reads = false;
  std::vector<std::string> extract_reads;  // --extract-reads A[,B,...]: the FASTQ files the bins are extracted from
  std::string compress = "plaintext";  // or "z"
  int compression_level = 6;           // 0 stores; 1 ... 9 run the core's one parse
  // --samples FILE / --devices d0[,d1,...]: a manifest of samples on resident handles, one worker per device entry
  bool have_samples = false, have_devices = false;
  std::string samples, devices;
  std::vector<std::string> given;  // the flags of msw_samples::conflicts() that the command line holds
  // --nested: the columns of -i are one hierarchy; the fields of its lines, and the flags of msw_nested::conflicts() given
  bool nested = false;
  std::vector<std::vector<std::string>> nested_rows;
  std::vector<std::string> nested_given;
};

// A message of the run to stderr, written whole when the object goes: under --samples the lines of two workers do not mix,
// and the worker's `sample <prefix>: ` (t_tag) stands in front of the message's first line.
thread_local std::string t_tag;
std::mutex g_err_mu;
struct Msg {
  std::ostringstream os;
  template <class T>
  Msg &operator<<(const T &v) {
    os << v;
    return *this;
  }
  ~Msg() {
    const std::string s = os.str();
    if (s.empty()) return;
    std::lock_guard<std::mutex> g(g_err_mu);
    std::cerr << t_tag << s;
    std::cerr.flush();
  }
};

std::vector<std::string> split(const std::string &s, char d) {
  std::vector<std::string> out;
  std::stringstream ss(s);
  std::string p;
  while (std::getline(ss, p, d)) out.push_back(p);
  return out;
}

Args parse(int argc, char **argv) {
  Args a;
  std::string t1, t2;
  for (int i = 1; i < argc; ++i) {
    const std::string k = argv[i];
    auto val = [&]() -> std::string {
      if (i + 1 >= argc) throw std::runtime_error("missing value for " + k);
      return argv[++i];
    };
    for (const std::string &f : msw_samples::conflicts())
      if (k == f) a.given.push_back(k);
    for (const std::string &f : msw_nested::conflicts())
      if (k == f) a.nested_given.push_back(k);
    if (k == "--themisto") a.themisto = split(val(), ',');
    else if (k == "--themisto-1") t1 = val();
    else if (k == "--themisto-2") t2 = val();
    else if (k == "--themisto-mode") a.mode = val();
    else if (k == "-i") a.indicators = val();
    else if (k == "-o") a.prefix = val();
    else if (k == "--iters") a.iters = std::stoul(val());
    else if (k == "--seed") a.seed = std::stoul(val());
    else if (k == "--bootstrap-count") a.bootstrap_count = std::stoul(val());
    else if (k == "--min-hits") a.min_hits = std::stoul(val());
    else if (k == "--max-iters") a.max_iters = std::stoul(val());
    else if (k == "-q") a.q = std::stod(val());
    else if (k == "-e") a.e = std::stod(val());
    else if (k == "--zero-inflation") a.zero_inflation = std::stod(val());
    else if (k == "--tol") a.tol = std::stod(val());
    else if (k == "--alphas") a.alphas = val();
    else if (k == "--algorithm") a.algorithm = val();
    else if (k == "--emprecision") a.emprecision = val();
    else if (k == "--gpu-index") a.gpu = std::stoi(val());
    else if (k == "-t") (void)val();  // host threads: nothing to set here
    else if (k == "--verbose") a.verbose = true;
    else if (k == "--nested") a.nested = true;
    else if (k == "--write-probs") a.write_probs = true;
    else if (k == "--print-probs") a.print_probs = true;
    else if (k == "--write-likelihood") a.write_likelihood = true;
    else if (k == "--write-likelihood-bitseq") a.write_likelihood_bitseq = true;
    else if (k == "--read-likelihood") a.read_likelihood = val();
    else if (k == "--no-fit-model") a.no_fit_model = true;
    else if (k == "--run-rate") a.run_rate = true;
    else if (k == "--bin-reads") a.bin_reads = true;
    else if (k == "--write-unassigned") a.write_unassigned = true;
    else if (k == "--write-assignment-table") a.write_assignment_table = true;
    else if (k == "--write-read-probs") a.write_read_probs = true;
    else if (k == "--probs-threshold") {
      a.probs_threshold = val();
      a.have_probs_threshold = true;
    }
    else if (k == "--compress") a.compress = val();
    else if (k == "--samples") {
      a.samples = val();
      a.have_samples = true;
    } else if (k == "--devices") {
      a.devices = val();
      a.have_devices = true;
    }
    else if (k == "--compression-level") a.compression_level = std::stoi(val());
    else if (k == "--target-groups") {
      a.target_groups = split(val(), ',');
      a.have_target_groups = true;
    } else if (k == "--extract-reads") {
      // (every element counts, an empty one too: main() refuses it)
      const std::string v = val();
      a.extract_reads.clear();
      for (size_t b = 0;;) {
        const size_t e = v.find(',', b);
        a.extract_reads.push_back(v.substr(b, e == std::string::npos ? e : e - b));
        if (e == std::string::npos) break;
        b = e + 1;
      }
      a.have_extract_reads = true;
    } else if (k == "--min-abundance") {
      a.min_abundance = std::stod(val());
      a.have_min_abundance = true;
    }
    else throw std::runtime_error("unknown argument " + k);
  }
  if (a.themisto.empty()) {
    if (!t1.empty()) a.themisto.push_back(t1);
    if (!t2.empty()) a.themisto.push_back(t2);
  }
  if (a.indicators.empty()) throw std::runtime_error("-i <group indicators> is required");
  return a;
}

// ConstructAdaptiveReference / AdaptiveGrouping::add_sequence (src/Reference.cpp:31-56,
// include/Grouping.hpp:75-80, include/Reference.hpp:67-94): one line per reference sequence, one grouping per
// tab-separated column, group ids in order of first appearance.  A line is split as repeated std::getline(..., '\t')
// splits it (Reference.hpp:74): an empty field between two tabs is a group named "", a trailing tab adds no field; an
// empty line stays one empty field (the group "" it has always been in a single-column file).  A line with another
// number of fields than the first is refused (the reference would end up with columns of different lengths).
struct Grouping {
  std::vector<std::string> names;
  std::vector<uint64_t> sizes;
  std::vector<uint32_t> indicators;
};
// the grouping a single-column file of these labels gives
Grouping grouping_of(const std::vector<std::string> &labels) {
  Grouping g;
  std::unordered_map<std::string, uint32_t> ids;
  for (const std::string &l : labels) {
    auto it = ids.find(l);
    if (it == ids.end()) {
      it = ids.emplace(l, (uint32_t)g.names.size()).first;
      g.names.push_back(l);
      g.sizes.push_back(0);
    }
    ++g.sizes[it->second];
    g.indicators.push_back(it->second);
  }
  return g;
}
// rows: when given, the fields of every line (--nested)
std::vector<Grouping> read_groupings(const std::string &path, std::vector<std::vector<std::string>> *rows = nullptr) {
  std::ifstream in(path);
  if (!in) throw std::runtime_error("cannot open " + path);
  std::vector<Grouping> gs;
  std::vector<std::unordered_map<std::string, uint32_t>> ids;
  std::string line;
  size_t n_lines = 0;
  while (std::getline(in, line)) {
    ++n_lines;
    std::vector<std::string> fields = split(line, '\t');
    if (fields.empty()) fields.emplace_back();
    if (n_lines == 1) {
      gs.resize(fields.size());
      ids.resize(fields.size());
    }
    if (fields.size() != gs.size())
      throw std::runtime_error("The grouping has " + std::to_string(fields.size()) + " columns on line " + std::to_string(n_lines) +
                               ", " + std::to_string(gs.size()) + " on line 1");
    if (rows) rows->push_back(fields);
    for (size_t c = 0; c < gs.size(); ++c) {
      Grouping &g = gs[c];
      auto it = ids[c].find(fields[c]);
      if (it == ids[c].end()) {
        it = ids[c].emplace(fields[c], (uint32_t)g.names.size()).first;
        g.names.push_back(fields[c]);
        g.sizes.push_back(0);
      }
      ++g.sizes[it->second];
      g.indicators.push_back(it->second);
    }
  }
  if (gs.empty()) throw std::runtime_error("The grouping contains 0 reference sequences");
  return gs;
}

// The file of an output of grouping `index` of K (src/OutfileDesignator.cpp:64-74,116-123): `<prefix>_<name>` for a
// single grouping, `<prefix>_<index>_<name>` when -i has several columns; without a prefix the bare name (the
// likelihood files: everything else goes to stdout then).  msweep_amd/reference.py output_path is the same function.
std::string out_path(const std::string &prefix, size_t index, size_t K, const std::string &name) {
  if (prefix.empty()) return name;
  return K > 1 ? prefix + "_" + std::to_string(index) + "_" + name : prefix + "_" + name;
}

void check(msw_handle h, int rc) {
  if (rc != 0) throw std::runtime_error(msw_last_error(h));
}

// An output of the run: a stream that is there already (stdout), a plain file, or -- --compress z -- `<path>.gz`
// (the extension is appended, as OutfileDesignator::open does, src/OutfileDesignator.cpp:30-62) whose bytes come from the
// one gzip stream the handle holds open: write takes host bytes (msw_core_gzip_append), text_block a block of a matrix
// output (msw_core_text_block_gzip).  The Python driver makes the same calls, so both write the same file.
class Out {
 public:
  Out(msw_handle h, std::ostream &os) : h_(h), os_(&os) {}
  Out(msw_handle h, const std::string &path, bool gz, int level) : h_(h), gz_(gz), os_(&file_) {
    if (!gz_) {
      file_.open(path);  // (a plain file that cannot be opened or written stays silent, as before --compress)
      return;
    }
    // the stream first: a refusal leaves no file behind
    const char *p = nullptr;
    size_t n = 0;
    check(h_, msw_core_gzip_begin(h_, level, &p, &n));
    open_ = true;
    file_.open(path + ".gz", std::ios::binary);
    if (!file_) throw std::runtime_error("cannot open " + path + ".gz");  // (~Out closes the stream)
    os_->write(p, (std::streamsize)n);
  }
  ~Out() {
    if (!open_) return;
    const char *p = nullptr;  // left open by a failure: the handle's stream is closed, the file is incomplete anyway
    size_t n = 0;
    (void)msw_core_gzip_end(h_, &p, &n);
  }
  void write(const char *p, size_t n) {
    if (!gz_) {
      os_->write(p, (std::streamsize)n);
      return;
    }
    constexpr size_t kPiece = (size_t)1 << 30;  // host bytes per msw_core_gzip_append call
    for (size_t o = 0; o < n; o += kPiece) {
      const char *z = nullptr;
      size_t nz = 0;
      check(h_, msw_core_gzip_append(h_, p + o, std::min(kPiece, n - o), &z, &nz));
      os_->write(z, (std::streamsize)nz);
    }
  }
  void write(const std::string &s) { write(s.data(), s.size()); }
  // the selection of a read file, whole records in pieces of at most max_bytes (msw_fastq_next / _next_gzip)
  void records(msw_fastq_t fq, size_t max_bytes) {
    for (;;) {
      const char *p = nullptr;
      size_t n = 0, n_text = 0;
      if (gz_) check(h_, msw_fastq_next_gzip(h_, fq, max_bytes, &p, &n, &n_text));
      else check(h_, msw_fastq_next(h_, fq, max_bytes, &p, &n));
      if (!(gz_ ? n_text : n)) break;
      os_->write(p, (std::streamsize)n);
    }
  }
  void text_block(int what, size_t e0, size_t e1, const uint64_t *prefix, size_t n_zero) {
    const char *p = nullptr;
    size_t n = 0;
    if (gz_) check(h_, msw_core_text_block_gzip(h_, what, e0, e1, prefix, n_zero, &p, &n, nullptr, nullptr));
    else check(h_, msw_core_text_block(h_, what, e0, e1, prefix, n_zero, &p, &n, nullptr));
    os_->write(p, (std::streamsize)n);
  }
  // the rows of the selection msw_core_sparse_probs_begin left, whole rows in pieces of at most max_bytes
  void sparse_rows(uint64_t n_rows, size_t max_bytes) {
    for (;;) {
      const char *p = nullptr;
      size_t n = 0;
      uint64_t done = 0;
      if (gz_) check(h_, msw_core_sparse_probs_next_gzip(h_, max_bytes, &p, &n, &done, nullptr));
      else check(h_, msw_core_sparse_probs_next(h_, max_bytes, &p, &n, &done, nullptr, nullptr));
      os_->write(p, (std::streamsize)n);
      if (done >= n_rows) break;
    }
  }
  // rows of the assignment table the handle keeps (msw_core_assign_table_block / _gzip)
  void table_block(size_t r0, size_t r1) {
    const char *p = nullptr;
    size_t n = 0;
    if (gz_) check(h_, msw_core_assign_table_block_gzip(h_, r0, r1, &p, &n, nullptr));
    else check(h_, msw_core_assign_table_block(h_, r0, r1, &p, &n));
    os_->write(p, (std::streamsize)n);
  }
  bool good() const { return (bool)*os_; }
  void close() {
    if (open_) {
      open_ = false;
      const char *p = nullptr;
      size_t n = 0;
      check(h_, msw_core_gzip_end(h_, &p, &n));
      os_->write(p, (std::streamsize)n);
    }
    os_->flush();
    if (gz_ && !*os_) throw std::runtime_error("writing the compressed file failed");
  }

 private:
  msw_handle h_;
  bool gz_ = false, open_ = false;
  std::ofstream file_;
  std::ostream *os_;
};

// a number as the reference's `*of << x` prints it (default ostream formatting: 6 significant digits)
std::string g6(double x) {
  char buf[64];
  snprintf(buf, sizeof buf, "%g", x);
  return buf;
}

// LL_WOR21::from_file (include/Likelihood.hpp:224-253): one line per equivalence class, `count \t L(0,j) ... L(G-1,j)`.
// The host parser: main() asks the device first (msw_core_set_dense_logl_file) and comes here for what it does not serve.
// A file that starts with the gzip magic is inflated through the library (msw_core_inflate_gzip: the kernels, or zlib).
void read_likelihood_file(msw_handle h, const std::string &path, size_t G, std::vector<uint64_t> &counts, std::vector<double> &L) {
  std::ifstream file(path, std::ios::binary);
  if (!file) throw std::runtime_error("Could not read from the likelihoods file.");
  std::istringstream inflated;
  const bool gz = file.get() == 0x1f && file.get() == 0x8b;
  file.clear();
  file.seekg(0);
  if (gz) {
    const std::string bytes((std::istreambuf_iterator<char>(file)), std::istreambuf_iterator<char>());
    const uint8_t *text = nullptr;
    size_t len = 0;
    msw_inflate_info info;
    if (msw_core_inflate_gzip(h, reinterpret_cast<const uint8_t *>(bytes.data()), bytes.size(), 0, &text, &len, &info))
      throw std::runtime_error("Could not read from the likelihoods file.");
    inflated.str(std::string(reinterpret_cast<const char *>(text), len));
  }
  std::istream &in = gz ? static_cast<std::istream &>(inflated) : file;
  std::vector<std::vector<double>> cols;
  std::string line;
  while (std::getline(in, line)) {
    const auto parts = split(line, '\t');
    if (parts.size() != G + 1) throw std::runtime_error("Could not read from the likelihoods file.");
    counts.push_back(std::stoull(parts[0]));
    std::vector<double> c(G);
    for (size_t g = 0; g < G; ++g) c[g] = std::stod(parts[g + 1]);
    cols.push_back(std::move(c));
  }
  const size_t E = cols.size();
  L.assign(G * E, 0.0);
  for (size_t j = 0; j < E; ++j)
    for (size_t g = 0; g < G; ++g) L[g * E + j] = cols[j][g];
}

// what the groupings of one run share: the handle and the alignment read once in front of the loop
struct Run {
  msw_handle h = nullptr;
  msw_alignment_t aln = nullptr;
  size_t n_ecs = 0, n_reads = 0, n_groupings = 1;
  std::vector<uint64_t> ec_counts;
  int algo = MSW_ALGO_RCG, prec = MSW_PREC_DOUBLE;
  // --extract-reads: the read files, opened at the first grouping that bins, and their record counts
  mutable std::vector<msw_fastq_t> fastqs;
  mutable std::vector<uint64_t> fastq_records;
  const Run *root = nullptr;  // --nested, below the root: the run that holds the read files and the sample's read count
};

// a node of the --nested walk: its stem and depth, and after its run the bins the descent takes
struct Node {
  std::string stem;
  size_t depth = 0;
  bool descend = false;
  std::vector<std::string> targets;
  std::vector<uint32_t> rows;
  std::vector<uint64_t> bin_ptr;
  std::vector<uint32_t> reads;
};

// ---- --bin-reads (src/mSWEEP.cpp:437-469; the same choices as msweep_amd/binning.py) ---------------------------------
struct BinningError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

// targets: every estimated group in group order, or --target-groups in the order given (a repeated name once); a
// name that is not an estimated group (unknown, or pruned by --min-hits) is refused.  --min-abundance m drops a
// target with theta < m (mGEMS::FilterTargetGroups), ties kept.  Returns the rows of the kept groups.
std::vector<uint32_t> bin_targets(const Args &a, const std::vector<std::string> &est, const std::vector<double> &theta,
                                  std::vector<std::string> &names, bool use_target_groups = true) {
  std::unordered_map<std::string, uint32_t> row;
  for (size_t i = 0; i < est.size(); ++i) row.emplace(est[i], (uint32_t)i);
  names.clear();
  for (const std::string &n : a.have_target_groups && use_target_groups ? a.target_groups : est) {
    if (!row.count(n)) throw BinningError("target group " + n + " is not among the estimated groups");
    if (std::find(names.begin(), names.end(), n) == names.end()) names.push_back(n);
  }
  std::vector<uint32_t> rows;
  std::vector<std::string> kept;
  for (const std::string &n : names) {
    const uint32_t r = row[n];
    if (a.have_min_abundance && theta[r] < a.min_abundance) continue;
    rows.push_back(r);
    kept.push_back(n);
  }
  names = std::move(kept);
  return rows;
}

// OutfileDesignator::bin (src/OutfileDesignator.cpp:80-93): `-o` up to its last '/', or '.', then /<name>.bin
std::string bin_path(const std::string &prefix, const std::string &name) {
  const size_t s = prefix.rfind('/');
  return (s == std::string::npos ? std::string(".") : prefix.substr(0, s)) + "/" + name + ".bin";
}

// min(16, hardware threads, the cgroup's CPU quota): the reader's rule (msweep_amd/csrc/host_alignment.inc)
size_t writer_threads() {
  size_t n = std::max<size_t>(1, std::min<size_t>(16, std::thread::hardware_concurrency()));
  if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
    char q[64] = {0};
    unsigned long long period = 0;
    if (fscanf(f, "%63s %llu", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0)
      n = std::max<size_t>(1, std::min<size_t>(n, (size_t)(strtoull(q, nullptr, 10) / period)));
    fclose(f);
  }
  return n;
}

// mGEMS::WriteBin: one decimal id per line, each line ending in '\n'; formatted with std::to_chars into 8 MB buffers.
// Returns an error text, empty on success.
std::string write_bin(const std::string &path, const uint32_t *ids, size_t n) {
  FILE *f = fopen(path.c_str(), "wb");
  if (!f) return "cannot open " + path + ": " + strerror(errno);
  constexpr size_t kBuf = 8u << 20;
  std::vector<char> buf(kBuf);
  size_t used = 0;
  std::string err;
  for (size_t i = 0; i < n && err.empty(); ++i) {
    if (kBuf - used < 16) {
      if (fwrite(buf.data(), 1, used, f) != used) err = "cannot write " + path + ": " + strerror(errno);
      used = 0;
    }
    char *e = std::to_chars(buf.data() + used, buf.data() + kBuf, ids[i]).ptr;
    *e++ = '\n';
    used = (size_t)(e - buf.data());
  }
  if (err.empty() && used && fwrite(buf.data(), 1, used, f) != used) err = "cannot write " + path + ": " + strerror(errno);
  if (fclose(f) != 0 && err.empty()) err = "cannot close " + path + ": " + strerror(errno);
  return err;
}

// --extract-reads: for the k-th FASTQ file (from 1) and every target group g, `<dir>/<g>_<k>.fastq` (`.fastq.gz`, one gzip
// stream, under --compress z) holds the records whose 0-based number in the file is a read id of g's bin, verbatim and in
// file order; an empty bin gives an empty file.  The files are opened at the first grouping that bins and stay resident on
// the device for the later ones (`fastqs`; main() closes them).  The same calls as msweep_amd/__main__.py extract_reads.
// Returns the exit status.
int extract_reads(const Args &a, msw_handle h, size_t n_reads, std::vector<msw_fastq_t> &fastqs, std::vector<uint64_t> &fastq_records,
                  const std::vector<std::string> &names, const std::vector<uint64_t> &bin_ptr, const std::vector<uint32_t> &reads) {
  constexpr size_t kPiece = (size_t)256 << 20;  // bytes of records per call
  try {
    if (fastqs.empty()) {
      static const char *const why[] = {"none", "forced", "header", "probe mismatch", "chunk status", "crc", "trailing bytes", "memory", "long span"};
      for (const std::string &path : a.extract_reads) {
        msw_fastq_t fq = nullptr;
        msw_fastq_info info;
        check(h, msw_fastq_open(h, path.c_str(), &fq, &info));
        fastqs.push_back(fq);
        fastq_records.push_back(info.n_records);
        if (a.verbose) {
          const msw_inflate_info &f = info.inflate;
          Msg m;
          m << "note: " << path << ": ";
          if (!f.payload_bytes && !f.fallback_reason) m << "plain text";
          else if (f.on_device && f.n_members) m << "gzip input inflated on the device (" << f.n_members << " BGZF members)";
          else if (f.on_device) m << "gzip input inflated on the device";
          else m << "gzip input inflated on the host (" << why[f.fallback_reason >= 0 && f.fallback_reason < 9 ? f.fallback_reason : 0] << ")";
          m << "; " << info.n_records << " records\n";
        }
      }
    }
    // before any file is written: a read file of another sample has another number of records
    for (size_t i = 0; i < fastqs.size(); ++i)
      if (fastq_records[i] != n_reads)
        throw std::runtime_error(a.extract_reads[i] + " holds " + std::to_string(fastq_records[i]) + " records, the pseudoalignment " +
                                 std::to_string(n_reads) + " reads");
    for (size_t i = 0; i < fastqs.size(); ++i)
      for (size_t k = 0; k < names.size(); ++k) {
        check(h, msw_fastq_select(h, fastqs[i], reads.data() + bin_ptr[k], bin_ptr[k + 1] - bin_ptr[k], nullptr, nullptr));
        const std::string bin = bin_path(a.prefix, names[k]);
        const std::string path = bin.substr(0, bin.size() - 4) + "_" + std::to_string(i + 1) + ".fastq";
        const bool gz = a.compress == "z";
        Out f(h, path, gz, a.compression_level);
        if (!gz && !f.good()) throw std::runtime_error("cannot open " + path);
        f.records(fastqs[i], kPiece);
        f.close();
        if (!f.good()) throw std::runtime_error("cannot write " + path);
      }
  } catch (const std::exception &ex) {
    Msg() << "Extracting the reads failed:\n  " << ex.what() << "\nexiting\n";
    return 1;
  }
  return 0;
}

int extract_after_bins(const Args &a, msw_handle h, const Run &r, const std::vector<std::string> &names,
                       const std::vector<uint64_t> &bin_ptr, const std::vector<uint32_t> &reads) {
  if (!a.have_extract_reads) return 0;
  const Run &top = r.root ? *r.root : r;  // (--nested: a child's bins hold the root's read ids)
  return extract_reads(a, h, top.n_reads, top.fastqs, top.fastq_records, names, bin_ptr, reads);
}

// --write-assignment-table: `#read_id` and the target names, then the rows of the table the device kept, a block of
// table_block_rows at a time (msweep_amd/binning.py: the same header, the same blocks)
void write_assignment_table(const Args &a, msw_handle h, const std::string &path, const std::vector<std::string> &targets) {
  Out f(h, path, a.compress == "z", a.compression_level);
  std::string head = "#read_id";
  for (const std::string &n : targets) head += "\t" + n;
  head += "\n";
  f.write(head);
  size_t n = 0;
  check(h, msw_core_assign_table_rows(h, &n));
  const size_t block = std::max<size_t>(1, std::min<size_t>((size_t)1 << 20, ((size_t)256 << 20) / (11 + 2 * targets.size())));
  for (size_t r0 = 0; r0 < n; r0 += block) f.table_block(r0, std::min(n, r0 + block));
  f.close();
  if (!f.good()) throw std::runtime_error("cannot write " + path);
}

// --write-read-probs / --probs-threshold: the refusals, in the words and the order of msweep_amd/read_probs.py; sets
// a.probs_tau.  Throws what main() prints as `Parsing arguments failed`.
void check_read_probs_flags(Args &a) {
  if (a.have_probs_threshold) {
    const std::string &t = a.probs_threshold;
    char *end = nullptr;
    double x = t.empty() || isspace((unsigned char)t[0]) ? NAN : strtod(t.c_str(), &end);
    if ((end && *end) || t.find_first_of("xX_") != std::string::npos) x = NAN;  // (decimal text only, as Python's float())
    if (!(x > 0.0 && x <= 1.0)) throw std::runtime_error("--probs-threshold must be a probability in (0, 1] (got " + t + ")");
    a.probs_tau = x;
    if (!a.write_read_probs) throw std::runtime_error("--probs-threshold needs --write-read-probs");
  }
  if (!a.write_read_probs) return;
  if (a.prefix.empty() && !a.have_samples) throw std::runtime_error("--write-read-probs needs -o");
  if (!a.read_likelihood.empty()) throw std::runtime_error("--write-read-probs can't be used with --read-likelihood");
  if (a.no_fit_model) throw std::runtime_error("--write-read-probs can't be used with --no-fit-model");
  if (a.nested) throw std::runtime_error("--write-read-probs can't be used with --nested");
}

// --write-read-probs: the header -- the threshold, one line per ESTIMATED group (g = its row in the resident likelihood, the
// number the rows carry), the column names --, then the rows the device selects and formats, one line per aligned read and
// group with probability >= --probs-threshold (msweep_amd/__main__.py write_read_probs: the same header, the same calls)
void write_read_probs(const Args &a, msw_handle h, msw_alignment_t aln, const std::string &path, const std::vector<std::string> &est,
                      const std::string &note) {
  Out f(h, path, a.compress == "z", a.compression_level);
  char num[64];
  snprintf(num, sizeof num, "%.17g", a.probs_tau);
  std::string head = std::string("#threshold\t") + num + "\n";
  for (size_t g = 0; g < est.size(); ++g) head += "#group\t" + std::to_string(g) + "\t" + est[g] + "\n";
  head += "#read_id\tgroup\tprob\n";
  f.write(head);
  uint64_t n_rows = 0;
  check(h, msw_core_sparse_probs_begin(h, aln, a.probs_tau, &n_rows, nullptr));
  f.sparse_rows(n_rows, (size_t)256 << 20);
  f.close();
  if (!f.good()) throw std::runtime_error("cannot write " + path);
  if (a.verbose) {
    uint64_t bytes = 0, cells = 0;
    check(h, msw_core_last_sparse_probs_timing(h, nullptr, &bytes, &cells));
    snprintf(num, sizeof num, "%g", a.probs_tau);
    Msg() << "note: " << note << "read probabilities: " << n_rows << " rows, " << cells << " cells at or above " << num << ", "
          << bytes << " bytes\n";
  }
}

// the bins from the device and one file per target (an empty bin: an empty file), written on up to writer_threads()
// threads, then --extract-reads; with --write-unassigned / --write-assignment-table the bins come from
// msw_core_assign_reads_aln, which judges every class against all estimated groups: one more bin, <dir>/unassigned_reads.bin,
// and the table.  Under --nested (`node`: the node of the walk) the bins are taken whether or not --bin-reads is given and
// stay on the node for the descent; below the root --min-abundance alone chooses the groups (--target-groups names level-0
// groups) and the files are `<dir>/<stem>_<group>.bin`.  Returns the exit status.
int bin_reads(const Args &a, msw_handle h, msw_alignment_t aln, const std::vector<std::string> &est,
              const std::vector<double> &theta, const Run &r, const std::string &table_path, const std::string &note,
              Node *node = nullptr) {
  std::vector<std::string> names, targets;
  std::vector<uint64_t> bin_ptr;
  std::vector<uint32_t> reads;
  const bool extras = a.write_unassigned || a.write_assignment_table;
  try {
    const std::vector<uint32_t> rows = bin_targets(a, est, theta, names, !node || node->depth == 0);
    targets = names;
    if (node) node->rows = rows;
    if (extras) {
      if (a.write_unassigned && std::find(est.begin(), est.end(), "unassigned_reads") != est.end())
        throw BinningError("a group is named unassigned_reads, the name of the file --write-unassigned writes");
      std::vector<double> thr(theta.size());
      for (size_t g = 0; g < theta.size(); ++g) thr[g] = 1.0 - theta[g];
      const unsigned unas = a.write_unassigned ? MSW_ASSIGN_UNASSIGNED : 0u;
      bin_ptr.assign(rows.size() + 1 + (a.write_unassigned ? 1 : 0), 0);
      uint64_t cls[3] = {0, 0, 0};
      check(h, msw_core_assign_reads_aln(h, aln, thr.data(), rows.data(), rows.size(), unas, bin_ptr.data(), nullptr, nullptr, nullptr));
      reads.resize(bin_ptr.back());
      check(h, msw_core_assign_reads_aln(h, aln, thr.data(), rows.data(), rows.size(),
                                         unas | (a.write_assignment_table ? MSW_ASSIGN_KEEP_TABLE : 0u), bin_ptr.data(), reads.data(),
                                         nullptr, cls));
      if (a.write_unassigned) names.push_back("unassigned_reads");  // the unassigned bin is the last one
      if (a.verbose)
        Msg() << "note: " << note << "reads assigned to one group: " << cls[1] << ", to several: " << cls[2]
                  << ", to none: " << cls[0] << ", of " << cls[0] + cls[1] + cls[2] << " aligned reads\n";
    } else {
      std::vector<double> thr(rows.size());
      for (size_t k = 0; k < rows.size(); ++k) thr[k] = 1.0 - theta[rows[k]];
      bin_ptr.assign(rows.size() + 1, 0);
      check(h, msw_core_bin_reads_aln(h, aln, rows.data(), thr.data(), rows.size(), bin_ptr.data(), nullptr, nullptr));
      reads.resize(bin_ptr.back());
      check(h, msw_core_bin_reads_aln(h, aln, rows.data(), thr.data(), rows.size(), bin_ptr.data(), reads.data(), nullptr));
    }
  } catch (const std::exception &ex) {
    Msg() << "Binning the reads failed:\n  " << ex.what() << "\nexiting\n";
    return 1;
  }
  if (node) {
    node->targets = targets;
    node->bin_ptr = bin_ptr;
    node->reads = reads;
    if (!a.bin_reads) return 0;
    for (std::string &nm : names) nm = msw_nested::bin_name(node->stem, nm);
  }
  const size_t n = names.size(), nt = std::min(n, writer_threads());
  std::vector<std::string> err(n);
  if (a.compress == "z") {
    // <dir>/<group>.bin.gz, one gzip stream after the other: the handle holds one at a time
    std::string ids;
    char num[16];
    for (size_t k = 0; k < n; ++k) {
      try {
        Out f(h, bin_path(a.prefix, names[k]), true, a.compression_level);
        ids.clear();
        for (uint64_t i = bin_ptr[k]; i < bin_ptr[k + 1]; ++i) {
          ids.append(num, (size_t)(std::to_chars(num, num + sizeof num, reads[i]).ptr - num));
          ids += '\n';
        }
        f.write(ids);
        f.close();
      } catch (const std::exception &ex) {
        Msg() << "Writing the bin for target group " << names[k] << " failed:\n  " << ex.what() << "\nexiting\n";
        return 1;
      }
    }
  } else {
    std::vector<std::thread> pool;
    for (size_t t = 0; t < nt; ++t)
      pool.emplace_back([&, t] {
        for (size_t k = t; k < n; k += nt)
          err[k] = write_bin(bin_path(a.prefix, names[k]), reads.data() + bin_ptr[k], bin_ptr[k + 1] - bin_ptr[k]);
      });
    for (auto &th : pool) th.join();
    for (size_t k = 0; k < n; ++k)
      if (!err[k].empty()) {
        Msg() << "Writing the bin for target group " << names[k] << " failed:\n  " << err[k] << "\nexiting\n";
        return 1;
      }
  }
  if (a.write_assignment_table) {
    try {
      write_assignment_table(a, h, table_path, targets);
    } catch (const std::exception &ex) {
      Msg() << "Writing the assignment table failed:\n  " << ex.what() << "\nexiting\n";
      return 1;
    }
  }
  return extract_after_bins(a, h, r, names, bin_ptr, reads);
}

// MSWEEP_HOST_TEXT=1 (developer switch): the matrices come to the host as doubles and are formatted here, cell by cell,
// as before the device formatter -- the other side of its A/B and of tests/test_gpu_cli_text.py
bool host_text() {
  const char *e = getenv("MSWEEP_HOST_TEXT");
  return e && e[0] == '1';
}
// classes per msw_core_text_block call: 8192, fewer when the worst-case text of a block (20 + cell * G + 2 n_zero + 12
// bytes per line) would exceed 256 MiB; MSWEEP_TEXT_BLOCK=n (developer switch) overrides it
size_t text_block_ecs(size_t n_groups, size_t n_zero, size_t cell) {
  const char *e = getenv("MSWEEP_TEXT_BLOCK");
  if (e && *e && std::strtoull(e, nullptr, 10) > 0) return (size_t)std::strtoull(e, nullptr, 10);
  const size_t per_line = 20 + cell * n_groups + 2 * n_zero + 12;
  return std::max<size_t>(1, std::min<size_t>(8192, ((size_t)256 << 20) / per_line));
}

// Sample::write_probs[2] (src/Sample.cpp:63-85,154-186): header `ec_id` + group names, one line per equivalence class
// of exp(gamma).  The lines are formatted on the device a block of classes at a time (msw_core_text_block,
// MSW_TEXT_PROBS); with MSWEEP_HOST_TEXT=1 the block comes as doubles (msw_core_gamma_block) and is formatted here.
void write_probs(Out &of, msw_handle h, const std::vector<std::string> &names, const std::vector<std::string> &zero_names,
                 size_t n_groups, size_t n_ecs) {
  std::string head = "ec_id";
  for (auto &n : names) head += '\t' + n;
  for (auto &n : zero_names) head += '\t' + n;
  of.write(head + '\n');
  if (host_text()) {
    const size_t block = 8192;
    std::vector<double> buf(n_groups * block);
    std::string s;
    for (size_t e0 = 0; e0 < n_ecs; e0 += block) {
      const size_t w = std::min(block, n_ecs - e0);
      check(h, msw_core_gamma_block(h, e0, e0 + w, buf.data(), w));
      s.clear();
      for (size_t jj = 0; jj < w; ++jj) {
        s += std::to_string(e0 + jj);
        for (size_t g = 0; g < n_groups; ++g) s += '\t' + g6(std::exp(buf[g * w + jj]));
        for (size_t z = 0; z < zero_names.size(); ++z) s += "\t0";
        s += '\n';
      }
      of.write(s);  // (one write per block: under --compress z a write is a call on the gzip stream)
    }
  } else {
    const size_t block = text_block_ecs(n_groups, zero_names.size(), 14);
    for (size_t e0 = 0; e0 < n_ecs; e0 += block) of.text_block(MSW_TEXT_PROBS, e0, std::min(n_ecs, e0 + block), nullptr, zero_names.size());
  }
  of.write("\n", 1);
  of.close();
}

// --write-likelihood (include/Likelihood.hpp:255-273): "count \t L(0,j) ... L(G-1,j)" per class, the lines formatted on
// the device (MSW_TEXT_LOGL): no G x E matrix on the host.  MSWEEP_HOST_TEXT=1: the dense matrix, formatted here.
void write_likelihood(Out &lf, msw_handle h, const std::vector<uint64_t> &ec_counts, size_t n_kept, size_t n_ecs) {
  if (host_text()) {
    std::vector<double> L(n_kept * n_ecs);
    check(h, msw_core_get_dense_logl(h, L.data(), n_ecs));
    std::string s;
    for (size_t e0 = 0; e0 < n_ecs; e0 += 8192) {
      s.clear();
      for (size_t j = e0; j < std::min(n_ecs, e0 + 8192); ++j) {
        s += std::to_string(ec_counts[j]);
        for (size_t g = 0; g < n_kept; ++g) s += '\t' + g6(L[g * n_ecs + j]);
        s += '\n';
      }
      lf.write(s);
    }
    lf.close();
    return;
  }
  const size_t block = text_block_ecs(n_kept, 0, 14);
  for (size_t e0 = 0; e0 < n_ecs; e0 += block) lf.text_block(MSW_TEXT_LOGL, e0, std::min(n_ecs, e0 + block), ec_counts.data() + e0, 0);
  lf.close();
}

// --write-likelihood-bitseq (include/Likelihood.hpp:275-311): five header lines, then one line per READ of every class --
// the read id (from 1, never restarting) and the class's tail, which the device formats once per class
// (MSW_TEXT_BITSEQ).  Ntotal / Nmap restate the reference's sum: std::accumulate starts from an `int` 0 with a lambda
// that returns a double, so the total is truncated to an integer after every class, and exp(log c) can fall just below
// c (a lone class of 5 reads gives 4): Ntotal can be below the number of reads.
void write_likelihood_bitseq(Out &lf, msw_handle h, const std::vector<uint64_t> &ec_counts, size_t n_kept, size_t n_ecs) {
  long long total = 0;
  for (uint64_t c : ec_counts) total = (long long)((double)total + std::exp(std::log((double)c)));
  lf.write("# Ntotal " + std::to_string(total) + "\n# Nmap " + std::to_string(total) + "\n# M " + std::to_string(n_kept) +
           "\n# LOGFORMAT (probabilities saved on log scale.)\n# r_name num_alignments (tr_id prob )^*{num_alignments}\n");
  uint64_t read_id = 1;
  const bool on_host = host_text();
  const size_t cell = 15 + std::to_string(n_kept + 1).size();
  const size_t block = on_host ? 8192 : text_block_ecs(n_kept, 0, cell);
  std::vector<double> buf;
  std::string tails, lines;
  for (size_t e0 = 0; e0 < n_ecs; e0 += block) {
    const size_t w = std::min(block, n_ecs - e0);
    const char *text = nullptr;
    size_t len = 0;
    if (on_host) {
      // (the likelihood itself has no block entry on the host side: the dense matrix, once)
      if (e0 == 0) {
        buf.resize(n_kept * n_ecs);
        check(h, msw_core_get_dense_logl(h, buf.data(), n_ecs));
      }
      tails.clear();
      for (size_t j = e0; j < e0 + w; ++j) {
        tails += std::to_string(n_kept + 1) + ' ';
        for (size_t g = 0; g < n_kept; ++g) tails += std::to_string(g + 1) + ' ' + g6(buf[g * n_ecs + j]) + ' ';
        tails += "0 -10000.00\n";
      }
      text = tails.data();
      len = tails.size();
    } else {
      check(h, msw_core_text_block(h, MSW_TEXT_BITSEQ, e0, e0 + w, nullptr, 0, &text, &len, nullptr));
    }
    const char *p = text, *end = text + len;
    lines.clear();  // (one write per block: under --compress z a write is a call on the gzip stream)
    for (size_t j = e0; j < e0 + w; ++j) {
      const char *nl = (const char *)std::memchr(p, '\n', (size_t)(end - p));
      if (!nl) throw std::runtime_error("the BitSeq text of a block ends before its last class");
      for (uint64_t k = 0; k < ec_counts[j]; ++k) {
        lines += std::to_string(read_id++);
        lines += ' ';
        lines.append(p, (size_t)(nl + 1 - p));
      }
      p = nl + 1;
    }
    lf.write(lines);
  }
  lf.close();
}

// digamma as the reference evaluates it (src/Sample.cpp:87-97)
double digamma_ref(double x) {
  double result = 0, xx, xx2, xx4;
  for (; x < 7; ++x) result -= 1 / x;
  x -= 1.0 / 2.0;
  xx = 1.0 / x;
  xx2 = xx * xx;
  xx4 = xx2 * xx2;
  result += std::log(x) + (1. / 24.) * xx2 - (7.0 / 960.0) * xx4 + (31.0 / 8064.0) * xx4 * xx2 - (127.0 / 30720.0) * xx4 * xx4;
  return result;
}
// Sample::dirichlet_kld + get_rates (src/Sample.cpp:99-152) on alphas_i = theta_i * sum c -- the column sums the solve
// already reduced on the device
void dirichlet_kld_rate(const std::vector<double> &alphas, std::vector<double> &kld, std::vector<double> &rate) {
  double a0 = 0.0;
  for (double a : alphas) a0 += a;
  std::vector<double> lk(alphas.size());
  double mx = 0.0;
  for (size_t i = 0; i < alphas.size(); ++i) {
    const double aj = alphas[i];
    const double v = std::lgamma(a0) - std::lgamma(a0 - aj) - std::lgamma(aj) + aj * (digamma_ref(aj) - digamma_ref(a0));
    lk[i] = std::log(std::max(v, 1e-16));
    mx = std::max(mx, lk[i]);
  }
  double s = 0.0;
  for (double v : lk) s += std::exp(v - mx);
  const double lsum = std::log(s) + mx;
  kld.resize(lk.size());
  rate.resize(lk.size());
  for (size_t i = 0; i < lk.size(); ++i) {
    kld[i] = std::exp(lk[i]);
    rate[i] = std::exp(lk[i] - lsum);
  }
}

// Everything main() does per grouping column -- the body of the loop at src/mSWEEP.cpp:282-563: the device build with
// this column's indicators (it replaces the resident likelihood and all that was derived from the one before,
// include/msweep_core.h), the likelihood outputs, the solve, the bins, the bootstrap, the probabilities and the
// abundances.  Returns the exit status (0: go on with the next grouping).
// node: the node of the --nested walk this run is (run_nested)
int run_grouping(const Args &a, const Run &r, const Grouping &grouping, size_t index, Node *node = nullptr) {
  msw_handle h = r.h;
  const size_t K = node ? 1 : r.n_groupings;
  // <prefix>_<name>, <prefix>_<index>_<name> when -i has several columns; --nested: <prefix>_<stem>_<name>
  auto path = [&](const std::string &name) {
    return node ? msw_nested::node_path(a.prefix, node->stem, name) : out_path(a.prefix, index, K, name);
  };
  const std::string note = K > 1 ? "grouping " + std::to_string(index) + ": " : std::string();  // --verbose
  const size_t G = grouping.names.size();
  size_t n_ecs = r.n_ecs, n_reads = r.n_reads, n_kept = 0;
  std::vector<uint64_t> file_counts;  // --read-likelihood: the first column of the file
  const std::vector<uint64_t> &ec_counts = a.read_likelihood.empty() ? r.ec_counts : file_counts;
  std::vector<uint8_t> mask(G, 1);
  std::vector<double> logc_file;  // --read-likelihood: the log counts of the file (the build leaves its own on the device)
  try {
    if (!a.read_likelihood.empty()) {
      // --read-likelihood (include/Likelihood.hpp:224-253): the dense matrix of a file through the dense boundary
      // -- parsed on the device where it serves the file (plain, gzip or BGZF), by read_likelihood_file otherwise
      msw_likfile_info lf;
      check(h, msw_core_set_dense_logl_file(h, a.read_likelihood.c_str(), G, &lf));
      if (a.verbose) {
        static const char *const why[] = {"none", "forced", "open / read", "bad byte", "bad token", "column count", "empty",
                                          "too many host cells", "range error", "memory", "too many lines"};
        Msg m;
        m << "note: " << note << a.read_likelihood << ": likelihood file parsed on ";
        if (lf.served) m << "the device (" << lf.n_host_cells << " cells on the host)\n";
        else m << "the host (" << why[lf.reason >= 0 && lf.reason < 11 ? lf.reason : 0] << ")\n";
      }
      if (lf.served) {
        n_ecs = (size_t)lf.n_ecs;
        file_counts.resize(n_ecs);
        check(h, msw_core_likfile_counts(h, file_counts.data(), n_ecs));
      } else {
        std::vector<double> L;
        read_likelihood_file(h, a.read_likelihood, G, file_counts, L);
        n_ecs = file_counts.size();
        if (n_ecs == 0) throw std::runtime_error("Could not read from the likelihoods file.");
        check(h, msw_core_set_dense_logl(h, L.data(), G, n_ecs, n_ecs));
      }
      n_kept = G;
      for (uint64_t c : file_counts) {
        logc_file.push_back(std::log((double)c));
        n_reads += c;   // (no alignment: the reads are those the file counts, as the Python mirror reports them)
      }
    } else {
      if (n_ecs == 0) throw std::runtime_error("no read aligned against the reference");
      check(h, msw_core_build_likelihood_aln(h, r.aln, grouping.indicators.data(), grouping.indicators.size(),
                                             grouping.sizes.data(), G, a.q, a.e, a.zero_inflation, a.min_hits, &n_kept,
                                             mask.data(), nullptr));
      // (the pseudoalignment stays: the next grouping is built from it, and --bin-reads reads its classes)
    }
  } catch (const std::exception &ex) {
    Msg() << "Building the log-likelihood array failed:\n  " << ex.what() << "\nexiting\n";
    return 1;
  }
  try {
    // written here if requested (src/mSWEEP.cpp:373-380: a failure has a message of its own)
    if (a.write_likelihood_bitseq) {
      // both likelihood flags: only the BitSeq file (src/mSWEEP.cpp:375-376)
      Out lf(h, path("bitseq_likelihoods.tsv"), a.compress == "z", a.compression_level);
      write_likelihood_bitseq(lf, h, ec_counts, n_kept, n_ecs);
    } else if (a.write_likelihood) {
      // --write-likelihood (include/Likelihood.hpp:255-273; the file: src/OutfileDesignator.cpp:67-74)
      Out lf(h, path("likelihoods.tsv"), a.compress == "z", a.compression_level);
      write_likelihood(lf, h, ec_counts, n_kept, n_ecs);
    }
  } catch (const std::exception &ex) {
    Msg() << "Writing the likelihood to file failed:\n  " << ex.what() << "\nexiting\n";
    return 1;
  }
  if (a.no_fit_model) return 0;  // src/mSWEEP.cpp:385-386
  std::vector<double> prior(n_kept, 1.0);
  if (!a.alphas.empty()) {
    // checked against THIS grouping's group count when it is reached (src/mSWEEP.cpp:392-396)
    const auto parts = split(a.alphas, ',');
    if (parts.size() != n_kept) {
      Msg() << "Error: --alphas must have the same number of values as there are groups.";
      return 1;
    }
    for (size_t i = 0; i < n_kept; ++i) prior[i] = std::stod(parts[i]);
  }
  uint64_t total = 0;
  for (uint64_t c : ec_counts) total += c;
  std::vector<std::string> est_names, zero_names;
  for (size_t g = 0; g < G; ++g) (mask[g] ? est_names : zero_names).push_back(grouping.names[g]);
  std::vector<std::vector<double>> results;  // [0] = estimate without resampling (include/Sample.hpp:157)
  try {
    std::vector<double> theta(n_kept);
    size_t it = 0;
    double bound = 0.0;
    // logc = NULL: the log counts stay where the build left them, on the device
    check(h, msw_core_solve(h, logc_file.empty() ? nullptr : logc_file.data(), prior.data(), a.tol, a.max_iters, r.algo, r.prec,
                            theta.data(), &it, &bound));
    if (a.verbose) {
      const size_t n = std::min<size_t>(it, 4096);
      std::vector<double> b(n), nn(n);
      size_t got = 0;
      check(h, msw_core_trace(h, n, b.data(), nn.data(), nullptr, nullptr, nullptr, &got));
      char buf[128];
      for (size_t k = 0; k < got; k += 5) {
        snprintf(buf, sizeof buf, "iter: %zu, bound: %g, |g|: %g\n", k, b[k], nn[k]);
        Msg() << "  " << note << buf;
      }
    }
    results.push_back(theta);
    if (a.bin_reads || (node && node->descend)) {
      // before the replicates and the probabilities (src/mSWEEP.cpp:437-469), from the point estimate
      if (bin_reads(a, h, r.aln, est_names, theta, r, path("reads_to_groups.tsv"), note, node) != 0) return 1;
    }
    if (a.write_read_probs) {
      // from the point estimate, before the replicates (a bootstrap drops the selection the device keeps)
      try {
        write_read_probs(a, h, r.aln, path("read_probs.tsv"), est_names, note);
      } catch (const std::exception &ex) {
        Msg() << "Writing the read probabilities failed:\n  " << ex.what() << "\nexiting\n";
        return 1;
      }
    }
    if (a.iters > 0) {
      // every grouping's bootstrap starts the stream from the same seed (the reference constructs the sample inside its
      // loop); the random-seed sentinel draws anew per grouping
      int32_t seed;
      if (a.seed == 26012023) {  // the reference's "random seed" sentinel (src/BootstrapSample.cpp:48-50)
        seed = (int32_t)(std::random_device{}() & 0x7fffffffu);
      } else {
        seed = (int32_t)(uint32_t)a.seed;  // size_t -> int32 narrowing (include/Sample.hpp:169)
      }
      // ConstructSample (src/Sample.cpp:30-50): --bootstrap-count is the number of draws with --bin-reads; the quirk
      // without it passes the number of ITERATIONS as the count
      const size_t draws = a.bootstrap_count > 0 ? (a.bin_reads ? a.bootstrap_count : a.iters) : (size_t)total;
      std::vector<uint32_t> w(ec_counts.begin(), ec_counts.end());
      std::vector<double> thetas(a.iters * n_kept);
      check(h, msw_core_bootstrap(h, w.data(), seed, draws, 0, a.iters, prior.data(), a.tol, a.max_iters, r.algo, r.prec,
                                  thetas.data(), nullptr));
      for (size_t b = 0; b < a.iters; ++b)
        results.emplace_back(thetas.begin() + b * n_kept, thetas.begin() + (b + 1) * n_kept);
    }
    // --write-probs / --print-probs: the probabilities of the un-resampled estimate (the replicates ran on solver
    // states of their own: the handle still holds it -- the reference writes them before its replicate loop,
    // src/mSWEEP.cpp:471-493)
    if (a.write_probs || a.print_probs) {
      const std::vector<std::string> none;
      const std::vector<std::string> &zn = a.min_hits > 0 ? zero_names : none;
      if (a.write_probs && !a.prefix.empty()) {
        Out pf(h, path("probs.tsv"), a.compress == "z", a.compression_level);
        write_probs(pf, h, est_names, zn, n_kept, n_ecs);
      }
      if (a.print_probs || (a.write_probs && a.prefix.empty())) {
        Out so(h, std::cout);
        write_probs(so, h, est_names, zn, n_kept, n_ecs);
      }
    }
  } catch (const std::exception &ex) {
    Msg() << "Estimating relative abundances failed:\n  " << ex.what() << "\nexiting\n";
    return 1;
  }

  // ---- abundances (default ostream formatting = 6 significant digits, as the reference) ----------
  std::ofstream file;
  if (!a.prefix.empty()) file.open(path("abundances.txt"));
  std::ostream &of = a.prefix.empty() ? std::cout : file;
  of << "#mSWEEP_version:\t" << kVersion << '\n' << "#num_reads:\t" << n_reads << '\n' << "#num_aligned:\t" << total << '\n';
  if (a.run_rate) {
    // experimental RATE / KLD (src/Sample.cpp:99-152; the table: src/mSWEEP.cpp:529-545)
    std::vector<double> alphas(n_kept), kld, rate;
    for (size_t i = 0; i < n_kept; ++i) alphas[i] = results[0][i] * (double)total;
    dirichlet_kld_rate(alphas, kld, rate);
    of << "#c_id\tmean_theta\tRATE\tKLD\n";
    for (size_t i = 0; i < n_kept; ++i)
      of << est_names[i] << '\t' << g6(results[0][i]) << '\t' << g6(rate[i]) << '\t' << g6(kld[i]) << '\n';
    for (auto &n : zero_names) of << n << "\t0\t0\t0\n";
    of.flush();
    return 0;
  }
  if (a.iters > 0) of << "#bootstrap_iters:\t" << a.iters << '\n' << "#c_id\tmean_theta\tbootstrap_mean_thetas\n";
  else of << "#c_id\tmean_theta\n";
  size_t row = 0;
  for (size_t g = 0; g < G; ++g) {  // estimated groups (all of them unless --min-hits pruned some)
    if (!mask[g]) continue;
    of << grouping.names[g];
    for (auto &res : results) of << '\t' << res[row];
    of << '\n';
    ++row;
  }
  if (a.min_hits > 0)
    for (size_t g = 0; g < G; ++g) {
      if (mask[g]) continue;
      of << grouping.names[g];
      for (size_t k = 0; k < results.size(); ++k) of << "\t0";
      of << '\n';
    }
  of.flush();
  return 0;
}

// One sample's pseudoalignment into r.  The reader runs ON THE DEVICE (msw_alignment_read_device: text -> equivalence
// classes in HBM) and the likelihood builds consume its arrays there (msw_core_build_likelihood_aln); only the classes'
// read counts come to the host.  Once per sample, in front of the grouping loop: the line count of -i is the same for
// every column.  Throws with the reference's messages.
void read_sample(const Args &a, Run &r, size_t n_targets) {
  msw_handle h = r.h;
  if (a.themisto.empty()) throw std::runtime_error("no pseudoalignment files given");
  if (a.mode != "intersection" && a.mode != "union") throw std::runtime_error("Unrecognized option `" + a.mode + "` for --themisto-mode");
  std::vector<const char *> paths;
  for (auto &p : a.themisto) paths.push_back(p.c_str());
  if (msw_alignment_read_device(h, paths.data(), paths.size(), n_targets, a.mode == "union" ? MSW_MERGE_UNION : MSW_MERGE_INTERSECTION,
                                &r.aln))
    throw std::runtime_error(msw_alignment_last_error());
  if (a.verbose) {
    // gzip input: inflated by the kernels, or by zlib where their result could not be vouched for
    static const char *const why[] = {"none", "forced", "header", "probe mismatch", "chunk status", "crc", "trailing bytes", "memory", "long span"};
    std::vector<msw_inflate_info> info(paths.size());
    size_t n_info = 0;
    if (msw_alignment_last_inflate(h, info.data(), info.size(), &n_info) == 0)
      for (size_t i = 0; i < std::min(n_info, info.size()); ++i) {
        if (!info[i].payload_bytes && !info[i].fallback_reason) continue;
        Msg m;
        m << "note: " << paths[i] << ": gzip input inflated on ";
        if (info[i].on_device && info[i].n_members) m << "the device (" << info[i].n_members << " BGZF members)\n";
        else if (info[i].on_device) m << "the device\n";
        else m << "the host (" << why[info[i].fallback_reason >= 0 && info[i].fallback_reason < 9 ? info[i].fallback_reason : 0] << ")\n";
      }
  }
  size_t n_hits = 0, n_aligned = 0;
  msw_alignment_shape(r.aln, &r.n_ecs, &r.n_reads, &n_hits, &n_aligned);
  r.ec_counts.resize(r.n_ecs);
  msw_alignment_export(r.aln, nullptr, nullptr, r.ec_counts.data(), nullptr, nullptr);
}

// --nested: the columns of -i as one tree, walked depth-first on the one handle.  A node runs the per-grouping body
// (run_grouping) on its alignment and the column of its depth; below depth K - 1 it then takes, for every binned group g in
// group order, the subset of its alignment with g's bin and the sequences labelled g (msw_alignment_subset: made on the
// device), forms the child grouping from the next column on exactly those -i lines, runs the child and
// destroys the child's alignment.  A child without a class, or whose sequences carry fewer than two groups in the next
// column, is skipped (--verbose says why).  A child that fails ends the run: its message carries `node <stem>: `.  The same
// steps as msweep_amd/__main__.py run_nested.
int run_nested_node(const Args &a, const Run &r, const Run &root, const std::vector<size_t> &lines, const std::vector<std::string> &names) {
  const auto &rows = a.nested_rows;
  const size_t K = rows[0].size(), depth = names.size();
  std::vector<std::string> labels;
  for (size_t i : lines) labels.push_back(rows[i][depth]);
  const Grouping grouping = grouping_of(labels);
  Node node;
  node.stem = msw_nested::stem(names);
  node.depth = depth;
  node.descend = depth + 1 < K;
  const std::string tag = t_tag;
  if (depth) t_tag += "node " + node.stem + ": ";
  const int rc = run_grouping(a, r, grouping, 0, &node);
  t_tag = tag;
  if (rc != 0 || !node.descend) return rc;
  std::vector<size_t> order(node.targets.size());
  for (size_t k = 0; k < order.size(); ++k) order[k] = k;
  std::vector<uint32_t> gid(order.size());
  for (size_t k = 0; k < order.size(); ++k)
    gid[k] = (uint32_t)(std::find(grouping.names.begin(), grouping.names.end(), node.targets[k]) - grouping.names.begin());
  std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return gid[x] < gid[y]; });  // group order
  for (size_t k : order) {
    const std::string &g = node.targets[k];
    std::vector<std::string> child = names;
    child.push_back(g);
    std::vector<uint8_t> keep(lines.size(), 0);
    std::vector<size_t> child_lines;
    std::vector<std::string> next;
    for (size_t j = 0; j < lines.size(); ++j)
      if (labels[j] == g) {
        keep[j] = 1;
        child_lines.push_back(lines[j]);
        if (std::find(next.begin(), next.end(), rows[lines[j]][depth + 1]) == next.end()) next.push_back(rows[lines[j]][depth + 1]);
      }
    if (next.size() < 2) {
      if (a.verbose)
        Msg() << "note: node " << msw_nested::stem(child) << ": skipped, its sequences carry fewer than two groups in column " << depth + 1
              << "\n";
      continue;
    }
    Run cr;
    cr.h = r.h;
    cr.n_groupings = 1;
    cr.algo = r.algo;
    cr.prec = r.prec;
    cr.root = &root;
    size_t n_keep = 0;
    if (msw_alignment_subset(r.h, r.aln, node.reads.data() + node.bin_ptr[k], node.bin_ptr[k + 1] - node.bin_ptr[k], keep.data(), &cr.aln,
                             &n_keep) != 0) {
      Msg() << "node " << msw_nested::stem(child) << ": Restricting the pseudoalignment failed:\n  " << msw_last_error(r.h) << "\nexiting\n";
      return 1;
    }
    size_t n_hits = 0, n_aligned = 0;
    msw_alignment_shape(cr.aln, &cr.n_ecs, &cr.n_reads, &n_hits, &n_aligned);
    int crc = 0;
    if (cr.n_ecs == 0) {
      if (a.verbose) Msg() << "note: node " << msw_nested::stem(child) << ": skipped, no read of its bin aligns against its sequences\n";
    } else {
      cr.ec_counts.resize(cr.n_ecs);
      msw_alignment_export(cr.aln, nullptr, nullptr, cr.ec_counts.data(), nullptr, nullptr);
      crc = run_nested_node(a, cr, root, child_lines, child);
    }
    msw_alignment_destroy(cr.aln);
    if (crc != 0) return crc;
  }
  return 0;
}

// the grouping loop, or under --nested the walk that takes its place: a grouping that fails ends the run, the files of the
// groupings before it stay
int run_all(const Args &a, const Run &r, const std::vector<Grouping> &groupings) {
  if (a.nested) {
    std::vector<size_t> lines(a.nested_rows.size());
    for (size_t i = 0; i < lines.size(); ++i) lines[i] = i;
    return run_nested_node(a, r, r, lines, {});
  }
  int rc = 0;
  for (size_t i = 0; i < groupings.size() && rc == 0; ++i) rc = run_grouping(a, r, groupings[i], i);
  return rc;
}

// Workers of --samples without --devices.  One: a second worker on the same device did not beat one by more than the
// spread of the repeats at both measured shapes (profiles/batch_timing.txt).
constexpr size_t kDefaultWorkers = 1;

// --samples: the manifest on resident handles.  Each worker owns one handle for its life, takes the next sample from the
// shared queue in manifest order, reads it, runs the grouping loop, closes its alignment and read files and trims the
// handle (msw_core_trim: one sample's reader temporaries do not stay under the next).  The first failure stops the queue:
// samples in flight finish, their files and those of the finished samples stay, the status is 1 -- after an error that may
// come from the device nothing more is started on it.  The same steps as msweep_amd/__main__.py run_samples.
int run_samples(const Args &a, const std::vector<msw_samples::Sample> &manifest, const std::vector<int> &devices) {
  std::vector<Grouping> groupings;
  try {
    groupings = read_groupings(a.indicators);
    if (a.verbose && groupings.size() > 1) std::cerr << "  read " << groupings.size() << " groupings\n";  // src/mSWEEP.cpp:265-267
  } catch (const std::exception &ex) {
    std::cerr << "Reading the pseudoalignments failed:\n  " << ex.what() << "\nexiting\n";
    return 1;
  }
  std::vector<msw_handle> handles;
  auto destroy_all = [&] {
    for (msw_handle h : handles) msw_core_destroy(h);
  };
  for (int d : devices) {
    msw_handle h = nullptr;
    if (msw_core_create(d, &h) != 0) {
      std::cerr << "Initialising the GPU failed:\n  " << msw_last_error(nullptr) << "\nexiting\n";
      destroy_all();
      return 1;
    }
    handles.push_back(h);
  }
  if (a.algorithm == "rcgcpu" && a.verbose)
    std::cerr << "note: --algorithm rcgcpu is served by the GPU RCG kernels (same algorithm as rcggpu)\n";
  const int algo = (a.algorithm == "rcggpu" || a.algorithm == "rcgcpu") ? MSW_ALGO_RCG : MSW_ALGO_EM;
  const int prec = a.emprecision == "float" ? MSW_PREC_FLOAT : MSW_PREC_DOUBLE;
  for (msw_handle h : handles)
    if (msw_core_set_pack_schedule(h, a.iters >= 5 ? 1 : 0) != 0) {
      std::cerr << "Building the log-likelihood array failed:\n  " << msw_last_error(h) << "\nexiting\n";
      destroy_all();
      return 1;
    }
  msw_samples::Queue queue(manifest.size());
  auto one = [&](msw_handle h, const msw_samples::Sample &s) -> int {
    Args sa = a;
    sa.prefix = s.prefix;
    sa.themisto = s.files;
    sa.have_extract_reads = s.have_fastqs;
    sa.extract_reads = s.fastqs;
    Run r;
    r.h = h;
    r.n_groupings = groupings.size();
    r.algo = algo;
    r.prec = prec;
    int rc = 0;
    try {
      try {
        read_sample(sa, r, groupings[0].indicators.size());
      } catch (const std::exception &ex) {
        Msg() << "Reading the pseudoalignments failed:\n  " << ex.what() << "\nexiting\n";
        rc = 1;
      }
      if (rc == 0) rc = run_all(sa, r, groupings);
    } catch (const std::exception &ex) {  // what a single run would end on uncaught: this sample's failure
      Msg() << "Running the sample failed:\n  " << ex.what() << "\nexiting\n";
      rc = 1;
    }
    for (msw_fastq_t fq : r.fastqs) msw_fastq_close(fq);
    msw_alignment_destroy(r.aln);
    if (rc == 0 && msw_core_trim(h) != 0) {
      Msg() << "Trimming the handle failed:\n  " << msw_last_error(h) << "\nexiting\n";
      rc = 1;
    }
    return rc;
  };
  std::vector<std::thread> workers;
  for (msw_handle h : handles)
    workers.emplace_back([&, h] {
      size_t i = 0;
      while (queue.next(i)) {
        t_tag = "sample " + manifest[i].prefix + ": ";
        const int rc = one(h, manifest[i]);
        t_tag.clear();
        queue.done(rc == 0);
      }
    });
  for (auto &w : workers) w.join();
  destroy_all();
  if (queue.failed() || a.verbose)
    std::cerr << "samples: " << queue.finished() << " finished, " << queue.failed() << " failed, " << queue.not_started()
              << " not started\n";
  return queue.failed() ? 1 : 0;
}

}  // namespace

int main(int argc, char **argv) {
  Args a;
  try {
    a = parse(argc, argv);
  } catch (const std::exception &ex) {
    std::cerr << "Parsing arguments failed:\n  " << ex.what() << "\nexiting\n";
    return 1;
  }
  std::vector<msw_samples::Sample> manifest;
  std::vector<int> devices;
  if (a.have_samples || a.have_devices) {
    // --samples: everything about the manifest is judged before the GPU is touched (samples_manifest.hpp)
    try {
      manifest = msw_samples::from_args(a.given, a.have_samples, a.samples, a.have_devices, a.devices, a.bin_reads, devices);
    } catch (const std::exception &ex) {
      std::cerr << "Parsing arguments failed:\n  " << ex.what() << "\nexiting\n";
      return 1;
    }
    if (devices.empty()) devices.assign(kDefaultWorkers, a.gpu);
  }
  // before the GPU is touched: the reference's words (src/OutfileDesignator.cpp:30-62) for what this core does not build
  if (a.compress != "plaintext" && a.compress != "z") {
    std::cerr << "Parsing arguments failed:\n  unsupported compression type " << a.compress
              << " (this core builds z only: gzip, compressed on the device)\nexiting\n";
    return 1;
  }
  if (a.compression_level < 0 || a.compression_level > 9) {
    std::cerr << "Parsing arguments failed:\n  unsupported compression level " << a.compression_level
              << " (this core builds z only, levels 0 ... 9)\nexiting\n";
    return 1;
  }
  if (a.prefix.empty() && !a.have_samples) a.compress = "plaintext";  // what goes to stdout stays plain
  if (a.bin_reads && !a.read_likelihood.empty()) {
    // "Can't be used with --bin-reads" (src/mSWEEP.cpp:115): the reads of a class are not in a likelihood file
    std::cerr << "Binning the reads failed:\n  --read-likelihood can't be used with --bin-reads\nexiting\n";
    return 1;
  }
  if ((a.write_unassigned || a.write_assignment_table) && !a.bin_reads) {
    // both go with the bins (--write-unassigned is named first when both are given)
    std::cerr << "Binning the reads failed:\n  " << (a.write_unassigned ? "--write-unassigned" : "--write-assignment-table")
              << " needs --bin-reads\nexiting\n";
    return 1;
  }
  if (a.have_extract_reads) {
    // --extract-reads: the bins are its input, and every path names a file
    if (!a.bin_reads) {
      std::cerr << "Extracting the reads failed:\n  --extract-reads needs --bin-reads\nexiting\n";
      return 1;
    }
    for (const std::string &p : a.extract_reads)
      if (p.empty()) {
        std::cerr << "Extracting the reads failed:\n  --extract-reads has an empty path in its list\nexiting\n";
        return 1;
      }
  }
  try {
    check_read_probs_flags(a);
  } catch (const std::exception &ex) {
    std::cerr << "Parsing arguments failed:\n  " << ex.what() << "\nexiting\n";
    return 1;
  }
  if (a.nested) {
    // --nested: the flags it refuses and the tree of -i are judged before the GPU is touched (nested_tree.hpp)
    try {
      msw_nested::check_flags(a.nested_given);
      try {
        read_groupings(a.indicators, &a.nested_rows);
      } catch (const std::exception &ex) {
        std::cerr << "Reading the pseudoalignments failed:\n  " << ex.what() << "\nexiting\n";
        return 1;
      }
      msw_nested::check_tree(a.indicators, a.nested_rows);
    } catch (const msw_nested::NestedError &ex) {
      std::cerr << "Parsing arguments failed:\n  " << ex.what() << "\nexiting\n";
      return 1;
    }
  }
  if (a.have_samples) return run_samples(a, manifest, devices);
  // every tab-separated column of -i is a grouping of its own; the estimation runs once per column
  // (src/mSWEEP.cpp:282), here from ONE resident alignment
  std::vector<Grouping> groupings;
  auto read_indicators = [&] {
    groupings = read_groupings(a.indicators);
    if (a.verbose && groupings.size() > 1) std::cerr << "  read " << groupings.size() << " groupings\n";  // src/mSWEEP.cpp:265-267
  };
  if (!a.read_likelihood.empty()) {
    // more than one grouping is refused in the reference's words (src/mSWEEP.cpp:360-362), before the GPU is touched:
    // with this flag the indicators are read first
    try {
      read_indicators();
    } catch (const std::exception &ex) {
      std::cerr << "Reading the pseudoalignments failed:\n  " << ex.what() << "\nexiting\n";
      return 1;
    }
    if (groupings.size() > 1) {
      std::cerr << "Reading the likelihoods failed:\n  Using more than one grouping with --read-likelihood is not yet implemented.\nexiting\n";
      return 1;
    }
  }
  Run r;
  if (msw_core_create(a.gpu, &r.h) != 0) {
    std::cerr << "Initialising the GPU failed:\n  " << msw_last_error(nullptr) << "\nexiting\n";
    return 1;
  }
  msw_handle h = r.h;
  try {
    if (groupings.empty()) read_indicators();
    r.n_groupings = groupings.size();
    // (--read-likelihood needs no pseudoalignments: src/mSWEEP.cpp:296-370)
    if (a.read_likelihood.empty()) read_sample(a, r, groupings[0].indicators.size());
  } catch (const std::exception &ex) {
    std::cerr << "Reading the pseudoalignments failed:\n  " << ex.what() << "\nexiting\n";
    msw_core_destroy(h);
    return 1;
  }
  if (a.algorithm == "rcgcpu" && a.verbose)  // the reference's default: the same RCG algorithm on the host; no CPU path here
    std::cerr << "note: --algorithm rcgcpu is served by the GPU RCG kernels (same algorithm as rcggpu)\n";
  r.algo = (a.algorithm == "rcggpu" || a.algorithm == "rcgcpu") ? MSW_ALGO_RCG : MSW_ALGO_EM;  // else em (src/mSWEEP.cpp:200)
  r.prec = a.emprecision == "float" ? MSW_PREC_FLOAT : MSW_PREC_DOUBLE;
  // (--emprecision float: fp32 kernels where the layout allows, msweep_amd/csrc/em_f32_kernels.hpp)
  int rc = 0;
  // ordering the cells for the LDS banks pays from about the 1 000th iteration on: bootstrap runs
  if (msw_core_set_pack_schedule(h, a.iters >= 5 ? 1 : 0) != 0) {
    std::cerr << "Building the log-likelihood array failed:\n  " << msw_last_error(h) << "\nexiting\n";
    rc = 1;
  }
  if (rc == 0) rc = run_all(a, r, groupings);
  // (the pseudoalignment goes at the end: device memory given back is scrubbed before it is handed out again, and the
  // solver state is allocated after the build)
  for (msw_fastq_t fq : r.fastqs) msw_fastq_close(fq);
  msw_alignment_destroy(r.aln);
  msw_core_destroy(h);
  return rc;
}
