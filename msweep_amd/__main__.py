"""`python -m msweep_amd` -- the estimation part of mSWEEP's command line (src/mSWEEP.cpp:68-148)
over the MI355X core: Themisto plaintext in, `<prefix>_abundances.txt` out, and with --bin-reads the
mGEMS bins `<dir>/<group>.bin` (src/mSWEEP.cpp:437-469; the bin pass runs on the device, msweep_amd/binning.py
holds the driver's side).  The matrix outputs -- --write-probs / --print-probs, --write-likelihood,
--write-likelihood-bitseq -- are formatted on the device (Core.text_block): only their bytes come to the host.
--compress z (src/mSWEEP.cpp:107-109, src/OutfileDesignator.cpp:30-62) writes them and the bins as `<name>.gz`, the
gzip stream compressed on the device as well (Core.gzip_begin / text_block_gzip / gzip_append / gzip_end); bz2, lzma
and zstd are refused, and --compression-level 1 ... 9 all run the core's one parse (0 stores).
--extract-reads A[,B,...] goes one step further than the bins: `<dir>/<group>_<k>.fastq` holds the binned reads of the k-th
FASTQ file themselves, gathered on the device where the file lies (Core.fastq_open; extract_reads below).
--write-unassigned / --write-assignment-table (with --bin-reads) add what `mGEMS bin` gives beyond the target bins:
`<dir>/unassigned_reads.bin`, the aligned reads no estimated group claims, and `<prefix>_reads_to_groups.tsv`, a 0/1 column
per target for every aligned read, formatted on the device (Core.assign_reads_aln / assign_table_block).
--write-read-probs / --probs-threshold x writes the probabilities per READ and sparse: `<prefix>_read_probs.tsv`, one line
`read id, group, probability` per aligned read and group at or above x, selected and formatted on the device
(Core.sparse_probs; write_read_probs below, msweep_amd/read_probs.py).
Every tab-separated column of the -i file is a grouping of its own: the estimation runs once per column
(src/mSWEEP.cpp:282) from ONE read of the pseudoalignment, and the files are `<prefix>_<i>_...` when there are several.
--samples FILE runs a whole manifest of samples (msweep_amd/samples.py) in this one process: -i is read once, every worker
(--devices, one per entry) keeps one handle for its life and takes the next sample from a shared queue, and each sample's
files are those a single run with its -o / --themisto / --extract-reads writes (run_samples below).
--nested makes the K >= 2 columns of -i ONE hierarchy, column 0 the coarsest: every node of the tree runs the per-grouping
body, and every bin of a node is estimated within its group from a sub-alignment made on the device
(Core.subset_alignment; run_nested below, msweep_amd/nested.py); files `<prefix>_<stem>_...`."""
import argparse
import copy
import math
import os
import sys
import threading

import numpy as np

from . import binning, nested, parallel, read_probs, samples
from .core import ALGO_EM, ALGO_RCG, PREC_DOUBLE, PREC_FLOAT, TEXT_BITSEQ, TEXT_LOGL, TEXT_PROBS, Core, MswError
from .likelihood import from_device_alignment, from_likelihood_file, read_likelihood_file  # noqa: F401 (read_likelihood_file: the host parser, under its name here)
from .reference import Grouping, _split, output_path, read_references
from .sample import BootstrapSample, PlainSample


def parse(argv):
    ap = argparse.ArgumentParser(prog="python -m msweep_amd")
    ap.add_argument("--themisto-1")
    ap.add_argument("--themisto-2")
    ap.add_argument("--themisto", help="comma separated list of alignment files")
    ap.add_argument("--themisto-mode", default="intersection")
    ap.add_argument("-i", required=True, dest="indicators")
    ap.add_argument("-o", default="", dest="prefix")
    ap.add_argument("-t", type=int, default=1, help="accepted for compatibility (the GPU core ignores it)")
    ap.add_argument("--max-iters", type=int, default=5000)
    ap.add_argument("--tol", type=float, default=0.000001)
    ap.add_argument("--algorithm", default="rcgcpu")   # the reference's default (src/mSWEEP.cpp:127); served by the GPU RCG kernels
    ap.add_argument("--emprecision", default="double")
    ap.add_argument("--iters", type=int, default=0)
    ap.add_argument("--seed", type=int, default=26012023)
    ap.add_argument("--bootstrap-count", type=int, default=0)
    ap.add_argument("-q", type=float, default=0.65)
    ap.add_argument("-e", type=float, default=0.01)
    ap.add_argument("--alphas")
    ap.add_argument("--zero-inflation", type=float, default=0.01)
    ap.add_argument("--min-hits", type=int, default=0)
    ap.add_argument("--run-rate", action="store_true")
    ap.add_argument("--write-probs", action="store_true")
    ap.add_argument("--print-probs", action="store_true")
    ap.add_argument("--write-likelihood", action="store_true")
    ap.add_argument("--write-likelihood-bitseq", action="store_true")
    ap.add_argument("--read-likelihood")
    ap.add_argument("--no-fit-model", action="store_true")
    ap.add_argument("--bin-reads", action="store_true")
    ap.add_argument("--target-groups", type=lambda v: v.split(","))
    ap.add_argument("--min-abundance", type=float)
    ap.add_argument("--extract-reads", type=lambda v: v.split(","),
                    help="FASTQ files A[,B,...] (plain, gzip or BGZF): with --bin-reads, <group>_<k>.fastq per target group and file")
    ap.add_argument("--write-unassigned", action="store_true",
                    help="with --bin-reads: <dir>/unassigned_reads.bin, the aligned reads no estimated group claims")
    ap.add_argument("--write-assignment-table", action="store_true",
                    help="with --bin-reads: <prefix>_reads_to_groups.tsv, a 0/1 column per target group for every aligned read")
    ap.add_argument("--write-read-probs", action="store_true",
                    help="<prefix>_read_probs.tsv: one line `read id, group, probability` per aligned read and group at or above "
                         "--probs-threshold, written on the device")
    ap.add_argument("--probs-threshold", help="with --write-read-probs: a probability in (0, 1] (default 0.001)")
    ap.add_argument("--compress", default="plaintext", help="plaintext or z (gzip, written on the device)")
    ap.add_argument("--compression-level", type=int, default=6, help="0 stores; 1 ... 9 run the same parse")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--samples", help="a manifest, one sample per line: <prefix> TAB <alignment files> [TAB <FASTQ files>]; "
                                      "takes the place of -o / --themisto / --extract-reads")
    ap.add_argument("--devices", help="with --samples: d0[,d1,...], one worker per entry (an entry may repeat)")
    ap.add_argument("--nested", action="store_true",
                    help="the K >= 2 columns of -i are one hierarchy, column 0 the coarsest: every bin of a node is estimated "
                         "within its group from a sub-alignment made on the device (files <prefix>_<stem>_...)")
    ap.add_argument("--verbose", action="store_true")
    return ap.parse_args(argv)


_SAY_LOCK = threading.Lock()


def _say(a, text):
    """A message of the run to stderr.  Under --samples it carries `sample <prefix>: ` in front of its first line and is
    written whole, so that the lines of two workers do not mix."""
    tag = getattr(a, "sample_tag", "")
    if not tag:
        sys.stderr.write(text)
        return
    with _SAY_LOCK:
        sys.stderr.write(tag + text)
        sys.stderr.flush()


def host_text():
    """MSWEEP_HOST_TEXT=1 (developer switch): the matrices come to the host as doubles and are formatted here, cell by
    cell, as before the device formatter -- the other side of its A/B and of tests/test_gpu_cli_text.py."""
    return os.environ.get("MSWEEP_HOST_TEXT", "") == "1"


def text_block_ecs(n_groups, n_zero=0, cell=14):
    """Classes per Core.text_block call: 8192, fewer when the worst-case text of a block (20 + cell * G + 2 n_zero + 12
    bytes per line) would exceed 256 MiB; MSWEEP_TEXT_BLOCK=n (developer switch) overrides it."""
    n = int(os.environ.get("MSWEEP_TEXT_BLOCK", "0") or 0)
    if n > 0:
        return n
    return max(1, min(8192, (256 << 20) // (20 + cell * n_groups + 2 * n_zero + 12)))


class GzipOut:
    """--compress z: `<path>.gz` (the extension is appended, as OutfileDesignator::open does, src/OutfileDesignator.cpp:30-62),
    its bytes from the one gzip stream the handle holds open.  write takes host bytes (Core.gzip_append), text_block a
    block of a matrix output (Core.text_block_gzip).  Both drivers make the same calls, so they write the same file."""
    PIECE = 1 << 30     # host bytes per gzip_append call

    def __init__(self, core, path, level):
        self.core = core
        head = core.gzip_begin(level)       # the stream first: a refusal leaves no file behind
        self.open = True
        try:
            self.f = open(path + ".gz", "wb")
        except OSError:
            self.open = False
            core.gzip_end()
            raise
        self.f.write(head)

    def write(self, data):
        """host bytes, or text (encoded), into the stream"""
        if isinstance(data, str):
            data = data.encode()
        for o in range(0, len(data), self.PIECE):
            self.f.write(self.core.gzip_append(data[o:o + self.PIECE]))

    def text_block(self, what, e0, e1, **kw):
        self.f.write(self.core.text_block_gzip(what, e0, e1, **kw))

    def table_block(self, r0, r1):
        self.f.write(self.core.assign_table_block_gzip(r0, r1))

    def pieces(self, pieces):
        """bytes the stream has given out already (Fastq.pieces_gzip)"""
        for z in pieces:
            self.f.write(z)

    def flush(self):
        pass

    def close(self):
        if self.open:
            self.open = False
            self.f.write(self.core.gzip_end())
        self.f.close()

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        try:
            self.close()
        except MswError:
            if exc_type is None:
                raise


def _open_out(core, path, a, mode="wb"):
    """an output file of the run: plain, or `<path>.gz` under --compress z"""
    return GzipOut(core, path, a.compression_level) if a.compress == "z" else open(path, mode)


def _text_block(f, core, what, e0, e1, **kw):
    if isinstance(f, GzipOut):
        f.text_block(what, e0, e1, **kw)
    else:
        f.write(core.text_block(what, e0, e1, **kw))


def _bytes_out(f):
    """where bytes go on a text stream (files opened here are binary already)"""
    if hasattr(f, "buffer"):
        f.flush()
        return f.buffer
    return f


def write_likelihood_file(f, ec_counts, lik):
    """--write-likelihood (include/Likelihood.hpp:255-273): "count \\t L(0,j) ... L(G-1,j)" per class, the lines
    formatted on the device (TEXT_LOGL): no G x E matrix on the host.  MSWEEP_HOST_TEXT=1: the dense matrix, here."""
    if host_text():
        L = lik.log_mat()
        for e0 in range(0, L.shape[1], 8192):
            f.write("".join(str(int(ec_counts[j])) + "\t" + "\t".join("%g" % x for x in L[:, j]) + "\n"
                            for j in range(e0, min(L.shape[1], e0 + 8192))).encode())
        return
    E, block = lik.n_ecs, text_block_ecs(lik.n_groups)
    counts = np.asarray(ec_counts, np.uint64)
    for e0 in range(0, E, block):
        e1 = min(E, e0 + block)
        _text_block(f, lik.core, TEXT_LOGL, e0, e1, line_prefix=counts[e0:e1])


def bitseq_total(ec_counts):
    """Ntotal / Nmap as the reference forms them (include/Likelihood.hpp:280-289): std::accumulate starts from an `int`
    0 with a lambda that returns a double, so the sum is truncated to an integer after every class -- and exp(log c)
    can fall just below c (a lone class of 5 reads gives 4).  Ntotal can therefore be below the number of reads."""
    acc = 0
    for c in ec_counts:
        acc = int(float(acc) + math.exp(math.log(float(c))))
    return acc


def write_likelihood_bitseq(f, ec_counts, lik):
    """--write-likelihood-bitseq (include/Likelihood.hpp:275-311): five header lines, then one line per READ of every
    class -- the read id (from 1, never restarting) and the class's tail, which the device formats once per class
    (TEXT_BITSEQ)."""
    G, E = lik.n_groups, lik.n_ecs
    total = bitseq_total(ec_counts)
    f.write((f"# Ntotal {total}\n# Nmap {total}\n# M {G}\n# LOGFORMAT (probabilities saved on log scale.)\n"
             "# r_name num_alignments (tr_id prob )^*{num_alignments}\n").encode())
    on_host = host_text()
    L = lik.log_mat() if on_host else None
    block = 8192 if on_host else text_block_ecs(G, 0, 15 + len(str(G + 1)))
    read_id = 1
    for e0 in range(0, E, block):
        e1 = min(E, e0 + block)
        if on_host:
            tails = [(f"{G + 1} " + "".join(f"{g + 1} {'%g' % x} " for g, x in enumerate(L[:, j])) + "0 -10000.00").encode()
                     for j in range(e0, e1)]
        else:
            tails = lik.core.text_block(TEXT_BITSEQ, e0, e1).split(b"\n")[:-1]
        if len(tails) != e1 - e0:
            raise RuntimeError("the BitSeq text of a block ends before its last class")
        lines = []      # (one write per block: under --compress z a write is a call on the gzip stream)
        for j, tail in zip(range(e0, e1), tails):
            c = int(ec_counts[j])
            lines.append(b"".join(str(read_id + k).encode() + b" " + tail + b"\n" for k in range(c)))
            read_id += c
        f.write(b"".join(lines))


def write_probs(of, names, zero_names, core, block=8192):
    """Sample::write_probs[2] (src/Sample.cpp:63-85,154-186), one line per EC.  The lines are formatted on the device a
    block of classes at a time (TEXT_PROBS); with MSWEEP_HOST_TEXT=1 the block comes as doubles (msw_core_gamma_block)
    and is formatted here.  The G x E matrix is never held, here or there.  `of`: a text stream, or a GzipOut."""
    of.write("ec_id\t" + "\t".join(list(names) + list(zero_names)) + "\n")
    G, E = core.shape()[:2]
    if host_text():
        for e0 in range(0, E, block):
            probs = np.exp(core.gamma_block(e0, min(E, e0 + block)))
            # (one write per block: under --compress z a write is a call on the gzip stream)
            of.write("".join(str(e0 + jj) + "\t" + "\t".join(["%g" % x for x in probs[:, jj]] + ["0"] * len(zero_names)) + "\n"
                             for jj in range(probs.shape[1])))
    else:
        raw = _bytes_out(of)
        block = text_block_ecs(G, len(zero_names))
        for e0 in range(0, E, block):
            _text_block(raw, core, TEXT_PROBS, e0, min(E, e0 + block), n_zero_cols=len(zero_names))
        raw.flush()
    of.write("\n")
    of.flush()


def _digamma(x):      # src/Sample.cpp:87-97
    r = 0.0
    while x < 7:
        r -= 1 / x
        x += 1
    x -= 0.5
    xx = 1.0 / x
    xx2 = xx * xx
    xx4 = xx2 * xx2
    return r + np.log(x) + (1. / 24.) * xx2 - (7.0 / 960.0) * xx4 + (31.0 / 8064.0) * xx4 * xx2 - (127.0 / 30720.0) * xx4 * xx4


def dirichlet_kld_rate(alphas):
    """Sample::dirichlet_kld + get_rates (src/Sample.cpp:99-152).  alphas_i = sum_j c_j exp(gamma_ij) is the
    column sum the solve already reduced on the device (theta_i * sum c)."""
    from math import lgamma
    a0 = float(np.sum(alphas))
    log_kld = np.array([np.log(max(lgamma(a0) - lgamma(a0 - aj) - lgamma(aj) + aj * (_digamma(aj) - _digamma(a0)), 1e-16))
                        for aj in map(float, alphas)])
    mx = max(0.0, float(log_kld.max()))
    lsum = np.log(np.exp(log_kld - mx).sum()) + mx
    return np.exp(log_kld), np.exp(log_kld - lsum)


EXTRACT_PIECE = 256 << 20     # bytes of records per Fastq.pieces call


def extract_reads(core, aln, targets, bin_ptr, reads, a, n_reads=None):
    """--extract-reads: for the k-th FASTQ file (from 1) and every target group g, `<dir>/<g>_<k>.fastq` (`.fastq.gz`, one
    gzip stream, under --compress z) holds the records whose 0-based number in the file is a read id of g's bin, verbatim
    and in file order; an empty bin gives an empty file.  The files are opened at the first grouping that bins, stay
    resident on the device for the later ones (a.fastqs) and go with the handle.  Returns the exit status."""
    try:
        if not a.fastqs:
            for path in a.extract_reads:
                fq = core.fastq_open(path)
                a.fastqs.append(fq)
                if a.verbose:
                    info = fq.info["inflate"]
                    if info["payload_bytes"] or info["fallback_reason"]:
                        how = "the device" if info["on_device"] else f"the host ({info['reason']})"
                        if info["on_device"] and info["n_members"]:
                            how += f" ({info['n_members']} BGZF members)"
                        _say(a, f"note: {path}: gzip input inflated on {how}; {fq.info['n_records']} records\n")
                    else:
                        _say(a, f"note: {path}: plain text; {fq.info['n_records']} records\n")
        # before any file is written: a read file of another sample has another number of records
        n_reads = aln.n_reads if n_reads is None else n_reads      # (--nested: a child's bins hold the root's read ids)
        for path, fq in zip(a.extract_reads, a.fastqs):
            if fq.info["n_records"] != n_reads:
                raise RuntimeError(f"{path} holds {fq.info['n_records']} records, the pseudoalignment {n_reads} reads")
        for k_file, fq in enumerate(a.fastqs, 1):
            for k, name in enumerate(targets):
                fq.select(reads[int(bin_ptr[k]):int(bin_ptr[k + 1])])
                out = binning.extract_path(a.prefix, name, k_file)
                if a.compress == "z":
                    with GzipOut(core, out, a.compression_level) as f:     # <dir>/<group>_<k>.fastq.gz
                        f.pieces(fq.pieces_gzip(EXTRACT_PIECE))
                else:
                    with open(out, "wb") as f:
                        for piece in fq.pieces(EXTRACT_PIECE):
                            f.write(piece)
    except (OSError, RuntimeError) as ex:      # (MswError is a RuntimeError)
        _say(a, f"Extracting the reads failed:\n  {ex}\nexiting\n")
        return 1
    return 0


def write_read_probs(core, aln, path, names, a, note=""):
    """--write-read-probs: the header (msweep_amd/read_probs.py), then the rows the device selects and formats
    (Core.sparse_probs by read: one line per aligned read and group with probability >= --probs-threshold), a piece of
    read_probs.PIECE bytes at a time: only bytes come to the host."""
    with _open_out(core, path, a) as f:
        f.write(read_probs.header(a.probs_tau, names))
        sp = core.sparse_probs(aln, a.probs_tau)
        if isinstance(f, GzipOut):
            f.pieces(sp.pieces_gzip(read_probs.PIECE))
        else:
            for piece in sp.pieces(read_probs.PIECE):
                f.write(piece)
        if a.verbose:
            _, nbytes, cells = sp.last_timing()
            _say(a, f"note: {note}read probabilities: {sp.rows} rows, {cells} cells at or above {a.probs_tau:g}, {nbytes} bytes\n")


def write_assignment_table(core, path, targets, a):
    """--write-assignment-table: `#read_id` and the target names, then the rows of the table the device kept
    (Core.assign_table_block), a block of binning.table_block_rows at a time: only bytes come to the host."""
    with _open_out(core, path, a) as f:
        f.write(binning.table_header(targets))
        n, block = core.assign_table_rows(), binning.table_block_rows(len(targets))
        for r0 in range(0, n, block):
            r1 = min(n, r0 + block)
            if isinstance(f, GzipOut):
                f.table_block(r0, r1)
            else:
                f.write(core.assign_table_block(r0, r1))


def bin_reads(core, aln, estimated_names, theta, a, table_path=None, note="", node=None):
    """--bin-reads (src/mSWEEP.cpp:437-469): targets, thresholds 1 - theta, the bins from the device, one file per
    target (an empty bin gives an empty file), then --extract-reads.  With --write-unassigned / --write-assignment-table
    the bins come from Core.assign_reads_aln, which judges every class against all estimated groups: one more bin for the
    reads nobody claims, and the table.  Under --nested (`node`: the node of the walk) the bins are taken whether or not
    --bin-reads is given and stay on the node for the descent; below the root --min-abundance alone chooses the groups
    (--target-groups names level-0 groups) and the files are `<dir>/<stem>_<group>.bin`.  Returns the exit status."""
    extras = a.write_unassigned or a.write_assignment_table
    try:
        targets = binning.resolve_targets(estimated_names, a.target_groups if node is None or node.depth == 0 else None)
        if a.min_abundance is not None:
            targets = binning.filter_min_abundance(targets, estimated_names, theta, a.min_abundance)
        row = {n: i for i, n in enumerate(estimated_names)}
        rows = [row[t] for t in targets]
        if extras:
            if a.write_unassigned:
                binning.check_unassigned_name(estimated_names)
            res = core.assign_reads_aln(aln, binning.all_thresholds(theta), rows, unassigned=a.write_unassigned,
                                        keep_table=a.write_assignment_table)
            bin_ptr, reads = res["bin_ptr"], res["reads"]
            if a.verbose:
                c0, c1, c2 = (int(x) for x in res["class_reads"])
                _say(a, f"note: {note}reads assigned to one group: {c1}, to several: {c2}, to none: {c0}, "
                                 f"of {c0 + c1 + c2} aligned reads\n")
        else:
            bin_ptr, reads, _ = core.bin_reads_aln(aln, rows, binning.thresholds(rows, theta))
    except (binning.BinningError, MswError) as ex:
        _say(a, f"Binning the reads failed:\n  {ex}\nexiting\n")
        return 1
    bins = list(targets) + ([binning.UNASSIGNED] if a.write_unassigned else [])    # the unassigned bin is the last one
    if node is not None:
        node.bins = (list(targets), rows, bin_ptr, reads)
        if not a.bin_reads:
            return 0
        bins = [nested.bin_name(node.stem, t) for t in targets]
    for k, name in enumerate(bins):
        try:
            ids = reads[int(bin_ptr[k]):int(bin_ptr[k + 1])]
            if a.compress == "z":
                with GzipOut(core, binning.bin_path(a.prefix, name), a.compression_level) as f:    # <dir>/<group>.bin.gz
                    f.write(binning.format_ids(ids))
            else:
                binning.write_bin(binning.bin_path(a.prefix, name), ids)
        except (OSError, MswError) as ex:
            _say(a, f"Writing the bin for target group {name} failed:\n  {ex}\nexiting\n")
            return 1
    if a.write_assignment_table:
        try:
            write_assignment_table(core, table_path, targets, a)
        except (OSError, MswError) as ex:
            _say(a, f"Writing the assignment table failed:\n  {ex}\nexiting\n")
            return 1
    if a.extract_reads:
        return extract_reads(core, aln, bins, bin_ptr, reads, a, None if node is None else node.root_reads)
    return 0


class Node:
    """a node of the --nested walk: its group names, and after its run the bins the descent takes"""

    def __init__(self, names, root_reads, descend):
        self.names, self.depth, self.stem = list(names), len(names), nested.stem(names)
        self.root_reads, self.descend, self.bins = root_reads, descend, None


def read_indicator_rows(a):
    """--nested: the fields of every line of -i (read_references has judged the file)"""
    with open(a.indicators) as f:
        read_references(f)
    with open(a.indicators) as f:
        return [_split(ln.rstrip("\n"), "\t") for ln in f]


def run_nested(a, core, aln, algo, prec):
    """--nested: the columns of -i as one tree, walked depth-first on the one handle.  A node runs the per-grouping body
    (run_grouping) on its alignment and the column of its depth; below depth K - 1 it then takes, for every binned group g
    in group order, the subset of its alignment with g's bin and the sequences labelled g (Core.subset_alignment: made on
    the device), forms the child grouping from the next column on exactly those -i lines, runs the child
    and closes the child's alignment.  A child without a class, or whose sequences carry fewer than two groups in the next
    column, is skipped (--verbose says why).  A child that fails ends the run: its message carries `node <stem>: `."""
    rows = a.nested_rows
    K = len(rows[0])

    def walk(node_aln, lines, names):
        depth = len(names)
        grouping = Grouping([rows[i][depth] for i in lines])
        node = Node(names, aln.n_reads, depth < K - 1)
        na = a
        if names:
            na = copy.copy(a)
            na.sample_tag = getattr(a, "sample_tag", "") + f"node {node.stem}: "
        rc = run_grouping(na, core, node_aln, grouping, 0, 1, algo, prec, node)
        if rc or not node.descend:
            return rc
        targets, trows, bin_ptr, reads = node.bins
        order = sorted(range(len(targets)), key=lambda k: grouping.name_to_id[targets[k]])      # group order
        labels = np.array([rows[i][depth] for i in lines], dtype=object)
        for k in order:
            g = targets[k]
            child = list(names) + [g]
            keep = labels == g
            child_lines = [i for i, kp in zip(lines, keep) if kp]
            if len({rows[i][depth + 1] for i in child_lines}) < 2:
                if a.verbose:
                    _say(a, f"note: node {nested.stem(child)}: skipped, its sequences carry fewer than two groups in column {depth + 1}\n")
                continue
            try:
                sub = core.subset_alignment(node_aln, reads[int(bin_ptr[k]):int(bin_ptr[k + 1])], keep.astype(np.uint8))
            except MswError as ex:
                _say(a, f"node {nested.stem(child)}: Restricting the pseudoalignment failed:\n  {ex}\nexiting\n")
                return 1
            try:
                if sub.n_ecs == 0:
                    if a.verbose:
                        _say(a, f"note: node {nested.stem(child)}: skipped, no read of its bin aligns against its sequences\n")
                    continue
                rc = walk(sub, child_lines, child)
                if rc:
                    return rc
            finally:
                sub.close()
        return 0
    return walk(aln, list(range(len(rows))), [])


def read_indicators(a):
    """every tab-separated column of -i is a grouping of its own (include/Reference.hpp:67-94); the estimation runs
    once per column (src/mSWEEP.cpp:282), from ONE resident alignment"""
    with open(a.indicators) as f:
        gs = read_references(f)
    if a.verbose and len(gs) > 1:
        sys.stderr.write(f"  read {len(gs)} groupings\n")      # src/mSWEEP.cpp:265-267
    return gs


def read_sample(a, core, files, n_targets):
    """The reader on the device (msw_alignment_read_device): text -> equivalence classes in HBM, consumed there by the
    likelihood build; the reference's messages for text it does not take.  Once per sample, in front of the grouping
    loop: the line count of -i is the same for every column."""
    if not files:
        raise RuntimeError("no pseudoalignment files given")
    aln = core.read_alignment(files, n_targets, a.themisto_mode)
    if a.verbose:
        # gzip input: inflated by the kernels, or by zlib where their result could not be vouched for
        for path, info in zip(files, core.last_inflate()):
            if info["payload_bytes"] or info["fallback_reason"]:
                how = "the device" if info["on_device"] else f"the host ({info['reason']})"
                if info["on_device"] and info["n_members"]:
                    how += f" ({info['n_members']} BGZF members)"
                _say(a, f"note: {path}: gzip input inflated on {how}\n")
    return aln


def run_groupings(a, core, aln, groupings, algo, prec):
    """The grouping loop (src/mSWEEP.cpp:282): build, outputs, solve, bins, bootstrap per column on the one handle -- every
    build replaces the resident likelihood and all that was derived from the one before (include/msweep_core.h).  A
    grouping that fails ends the sample; the files of the groupings before it stay.  Returns the exit status."""
    try:
        if a.nested:
            return run_nested(a, core, aln, algo, prec)      # the walk takes the place of the loop
        for index, grouping in enumerate(groupings):
            rc = run_grouping(a, core, aln, grouping, index, len(groupings), algo, prec)
            if rc:
                return rc
    finally:
        for fq in list(a.fastqs):      # --extract-reads: the read files go at the end of the sample
            fq.close()
    return 0


def _algo_prec(a):
    algo = ALGO_RCG if a.algorithm in ("rcggpu", "rcgcpu") else ALGO_EM   # anything else -> em (src/mSWEEP.cpp:200)
    # (--emprecision float: fp32 kernels where the layout allows, msweep_amd/csrc/em_f32_kernels.hpp; the library
    # reports which through msw_timing::em_float_kernels)
    return algo, PREC_FLOAT if a.emprecision == "float" else PREC_DOUBLE


# Workers of --samples without --devices.  One: a second worker on the same device did not beat one by more than the
# spread of the repeats at both measured shapes (profiles/batch_timing.txt).
DEFAULT_WORKERS = 1


def run_samples(a, manifest, devices):
    """--samples: the manifest on resident handles.  Each worker owns one handle for its life, takes the next sample from
    the shared queue in manifest order, reads it, runs the grouping loop, closes its alignment and read files and trims
    the handle (msw_core_trim: one sample's reader temporaries do not stay under the next).  The first failure stops the
    queue: samples in flight finish, their files and those of the finished samples stay, the status is 1 -- after an
    error that may come from the device nothing more is started on it."""
    try:
        groupings = read_indicators(a)
    except (RuntimeError, OSError) as ex:
        sys.stderr.write(f"Reading the pseudoalignments failed:\n  {ex}\nexiting\n")
        return 1
    cores = []
    try:
        for d in devices:
            cores.append(Core(d))
    except MswError as ex:
        sys.stderr.write(f"Initialising the GPU failed:\n  {ex}\nexiting\n")
        return 1
    if a.algorithm == "rcgcpu" and a.verbose:
        sys.stderr.write("note: --algorithm rcgcpu is served by the GPU RCG kernels (same algorithm as rcggpu)\n")
    algo, prec = _algo_prec(a)
    try:
        for core in cores:
            core.set_pack_schedule(a.iters >= 5)
    except MswError as ex:
        sys.stderr.write(f"Building the log-likelihood array failed:\n  {ex}\nexiting\n")
        return 1
    lock = threading.Lock()
    state = {"next": 0, "finished": 0, "failed": 0}
    n_targets = len(groupings[0].group_indicators)

    def one(core, s):
        sa = copy.copy(a)
        sa.prefix, sa.extract_reads, sa.fastqs, sa.sample_tag = s.prefix, s.fastqs, [], f"sample {s.prefix}: "
        try:
            try:
                aln = read_sample(sa, core, s.files, n_targets)
            except (RuntimeError, OSError, MswError) as ex:
                _say(sa, f"Reading the pseudoalignments failed:\n  {ex}\nexiting\n")
                return 1
            try:
                return run_groupings(sa, core, aln, groupings, algo, prec)
            finally:
                aln.close()
        except Exception as ex:      # what a single run would end on with a traceback: this sample's failure
            _say(sa, f"Running the sample failed:\n  {type(ex).__name__}: {ex}\nexiting\n")
            return 1

    def worker(core):
        while True:
            with lock:
                if state["failed"] or state["next"] >= len(manifest):
                    return
                s = manifest[state["next"]]
                state["next"] += 1
            rc = one(core, s)
            if rc == 0:
                try:
                    core.trim()
                except MswError as ex:
                    _say(a, f"sample {s.prefix}: Trimming the handle failed:\n  {ex}\nexiting\n")
                    rc = 1
            with lock:
                state["failed" if rc else "finished"] += 1

    threads = [threading.Thread(target=worker, args=(core,)) for core in cores]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for core in cores:
        core.close()
    if state["failed"] or a.verbose:
        sys.stderr.write(f"samples: {state['finished']} finished, {state['failed']} failed, "
                         f"{len(manifest) - state['finished'] - state['failed']} not started\n")
    return 1 if state["failed"] else 0


def main(argv=None):
    a = parse(sys.argv[1:] if argv is None else argv)
    aln = None
    manifest = None
    if a.samples is not None or a.devices is not None:
        # --samples: everything about the manifest is judged before the GPU is touched (msweep_amd/samples.py)
        given = [f for f, v in (("--themisto", a.themisto), ("--themisto-1", a.themisto_1), ("--themisto-2", a.themisto_2),
                                ("-o", a.prefix), ("--read-likelihood", a.read_likelihood), ("--print-probs", a.print_probs),
                                ("--extract-reads", a.extract_reads is not None)) if v]
        try:
            manifest, devices = samples.from_args(given, a.samples, a.devices, a.bin_reads)
        except samples.ManifestError as ex:
            sys.stderr.write(f"Parsing arguments failed:\n  {ex}\nexiting\n")
            return 1
        if devices is None:
            devices = [a.device] * DEFAULT_WORKERS
    # before the GPU is touched: the reference's words (src/OutfileDesignator.cpp:30-62) for what this core does not build
    if a.compress not in ("plaintext", "z"):
        sys.stderr.write(f"Parsing arguments failed:\n  unsupported compression type {a.compress} "
                         "(this core builds z only: gzip, compressed on the device)\nexiting\n")
        return 1
    if not 0 <= a.compression_level <= 9:
        sys.stderr.write(f"Parsing arguments failed:\n  unsupported compression level {a.compression_level} "
                         "(this core builds z only, levels 0 ... 9)\nexiting\n")
        return 1
    if not a.prefix and manifest is None:
        a.compress = "plaintext"        # what goes to stdout stays plain
    if a.bin_reads and a.read_likelihood:
        # "Can't be used with --bin-reads" (src/mSWEEP.cpp:115): the reads of a class are not in a likelihood file
        sys.stderr.write("Binning the reads failed:\n  --read-likelihood can't be used with --bin-reads\nexiting\n")
        return 1
    for flag, on in (("--write-unassigned", a.write_unassigned), ("--write-assignment-table", a.write_assignment_table)):
        if on and not a.bin_reads:
            sys.stderr.write(f"Binning the reads failed:\n  {flag} needs --bin-reads\nexiting\n")
            return 1
    if a.extract_reads is not None:
        # --extract-reads: the bins are its input, and every path names a file
        if not a.bin_reads:
            sys.stderr.write("Extracting the reads failed:\n  --extract-reads needs --bin-reads\nexiting\n")
            return 1
        if any(not p for p in a.extract_reads):
            sys.stderr.write("Extracting the reads failed:\n  --extract-reads has an empty path in its list\nexiting\n")
            return 1
    try:
        # --write-read-probs / --probs-threshold (msweep_amd/read_probs.py)
        a.probs_tau = read_probs.check_flags(a.write_read_probs, a.probs_threshold, bool(a.prefix), manifest is not None,
                                             bool(a.read_likelihood), a.no_fit_model, a.nested)
    except read_probs.ReadProbsError as ex:
        sys.stderr.write(f"Parsing arguments failed:\n  {ex}\nexiting\n")
        return 1
    if a.nested:
        # --nested: the flags it refuses and the tree of -i are judged before the GPU is touched (msweep_amd/nested.py)
        given = [f for f, v in (("--read-likelihood", a.read_likelihood), ("--no-fit-model", a.no_fit_model), ("--alphas", a.alphas),
                                ("--write-unassigned", a.write_unassigned), ("--write-assignment-table", a.write_assignment_table),
                                ("--print-probs", a.print_probs)) if v]
        try:
            nested.check_flags(given)
            try:
                a.nested_rows = read_indicator_rows(a)
            except (RuntimeError, OSError) as ex:
                sys.stderr.write(f"Reading the pseudoalignments failed:\n  {ex}\nexiting\n")
                return 1
            nested.check_tree(a.indicators, a.nested_rows)
        except nested.NestedError as ex:
            sys.stderr.write(f"Parsing arguments failed:\n  {ex}\nexiting\n")
            return 1
    if manifest is not None:
        return run_samples(a, manifest, devices)
    a.fastqs = []     # the read files of --extract-reads, resident from the first grouping that bins
    groupings = None
    if a.read_likelihood:
        # more than one grouping is refused in the reference's words (src/mSWEEP.cpp:360-362), before the GPU is touched:
        # with this flag the indicators are read first
        try:
            groupings = read_indicators(a)
        except (RuntimeError, OSError) as ex:
            sys.stderr.write(f"Reading the pseudoalignments failed:\n  {ex}\nexiting\n")
            return 1
        if len(groupings) > 1:
            sys.stderr.write("Reading the likelihoods failed:\n  Using more than one grouping with --read-likelihood is not yet "
                             "implemented.\nexiting\n")
            return 1
    try:
        core = Core(a.device)
    except MswError as ex:
        sys.stderr.write(f"Initialising the GPU failed:\n  {ex}\nexiting\n")
        return 1
    try:
        if groupings is None:
            groupings = read_indicators(a)
        if not a.read_likelihood:
            files = a.themisto.split(",") if a.themisto else [x for x in (a.themisto_1, a.themisto_2) if x]
            aln = read_sample(a, core, files, len(groupings[0].group_indicators))
    except (RuntimeError, OSError, MswError) as ex:
        sys.stderr.write(f"Reading the pseudoalignments failed:\n  {ex}\nexiting\n")
        return 1
    if a.algorithm == "rcgcpu":
        # the reference's default: the same RCG algorithm on the host (rcgpar::rcg_optl_omp); this core runs it
        # on the GPU -- there is no CPU path here
        if a.verbose:
            sys.stderr.write("note: --algorithm rcgcpu is served by the GPU RCG kernels (same algorithm as rcggpu)\n")
    algo, prec = _algo_prec(a)
    try:
        # ordering the cells for the LDS banks pays from about the 1 000th iteration on: bootstrap runs (msw_core_set_pack_schedule)
        core.set_pack_schedule(a.iters >= 5)
    except MswError as ex:
        sys.stderr.write(f"Building the log-likelihood array failed:\n  {ex}\nexiting\n")
        return 1
    rc = run_groupings(a, core, aln, groupings, algo, prec)
    if rc:
        return rc
    core.close()
    return 0


def run_grouping(a, core, aln, grouping, index, K, algo, prec, node=None):
    """Everything main() does per grouping column: the body of the loop at src/mSWEEP.cpp:282-563.  Returns the exit
    status (0: go on with the next grouping).  node: the node of the --nested walk this run is (run_nested)."""
    def path(name):      # <prefix>_<name>, <prefix>_<index>_<name> when -i has several columns; --nested: <prefix>_<stem>_<name>
        if node is not None:
            return nested.node_path(a.prefix, node.stem, name)
        return output_path(a.prefix, index, K, name)
    note = f"grouping {index}: " if K > 1 else ""     # --verbose: in front of the notes of a grouping
    try:
        if a.read_likelihood:
            # --read-likelihood (include/Likelihood.hpp:224-253): "count \t L(0,j) ... L(G-1,j)" per EC
            # -- parsed on the device where it serves the file (plain, gzip or BGZF), by read_likelihood_file otherwise
            lik = from_likelihood_file(core, a.read_likelihood, grouping.get_n_groups())
            ec_counts, info = lik.ec_counts, lik.file_info
            if a.verbose:
                how = f"the device ({info['n_host_cells']} cells on the host)" if info["served"] else f"the host ({info['reason_text']})"
                _say(a, f"note: {note}{a.read_likelihood}: likelihood file parsed on {how}\n")
            n_reads = total_reads = int(ec_counts.sum())
        else:
            if aln.n_ecs == 0:
                raise RuntimeError("no read aligned against the reference")
            lik = from_device_alignment(core, aln, grouping.group_indicators, grouping.get_sizes(), a.q, a.e,
                                        a.zero_inflation, a.min_hits)
            ec_counts = aln.ec_counts()
            n_reads = aln.n_reads
    except (MswError, RuntimeError, OSError, ValueError) as ex:
        _say(a, f"Building the log-likelihood array failed:\n  {ex}\nexiting\n")
        return 1
    try:
        if a.write_likelihood_bitseq:
            # both likelihood flags: only the BitSeq file (src/mSWEEP.cpp:375-376); <prefix>_bitseq_likelihoods.tsv
            # (src/OutfileDesignator.cpp:67-74)
            with _open_out(core, path("bitseq_likelihoods.tsv"), a) as f:
                write_likelihood_bitseq(f, ec_counts, lik)
        elif a.write_likelihood:
            # --write-likelihood (include/Likelihood.hpp:255-273), default ostream precision; the file is
            # <prefix>_likelihoods.tsv (src/OutfileDesignator.cpp:67-74; the flag's help text says .txt)
            with _open_out(core, path("likelihoods.tsv"), a) as f:
                write_likelihood_file(f, ec_counts, lik)
    except (MswError, RuntimeError, OSError) as ex:
        _say(a, f"Writing the likelihood to file failed:\n  {ex}\nexiting\n")
        return 1
    if a.no_fit_model:
        return 0
    G = lik.n_groups
    prior = np.ones(G)
    if a.alphas:
        prior = np.array([float(x) for x in a.alphas.split(",")])
        if len(prior) != G:
            _say(a, "Error: --alphas must have the same number of values as there are groups.")
            return 1
    total = int(ec_counts.sum())
    sample = BootstrapSample(n_reads, total, a.iters) if a.iters > 0 else PlainSample(n_reads, total)
    try:
        # a likelihood built on the device keeps its log counts there: nothing to upload per solve
        res = core.solve(None if not a.read_likelihood else lik.log_counts(), prior, a.tol, a.max_iters, algo, prec)
        if a.verbose:
            t = core.trace(min(res["iters"], 4096))
            for k in range(0, t["n"], 5):
                _say(a, f"  {note}iter: {k}, bound: {t['bound'][k]:g}, |g|: {t['newnorm'][k]:g}\n")
        sample.store_abundances(res["theta"])
    except MswError as ex:
        _say(a, f"Estimating relative abundances failed:\n  {ex}\nexiting\n")
        return 1
    if a.bin_reads or (node is not None and node.descend):
        # before the replicates and the probabilities (src/mSWEEP.cpp:437-469), from the point estimate
        est = [n for n, m in zip(grouping.get_names(), lik.groups_considered()) if m]
        rc = bin_reads(core, aln, est, res["theta"], a, path("reads_to_groups.tsv"), note, node)
        if rc:
            return rc
    if a.write_read_probs:
        # from the point estimate, before the replicates (a bootstrap drops the selection the device keeps)
        try:
            write_read_probs(core, aln, path("read_probs.tsv"), [n for n, m in zip(grouping.get_names(), lik.groups_considered()) if m],
                             a, note)
        except (MswError, RuntimeError, OSError) as ex:
            _say(a, f"Writing the read probabilities failed:\n  {ex}\nexiting\n")
            return 1
    try:
        if a.iters > 0:
            if a.seed == 26012023:      # the reference's "random seed" sentinel (src/BootstrapSample.cpp:48-50)
                seed = int(np.random.SeedSequence().generate_state(1)[0] & 0x7fffffff)
            else:
                seed = ((a.seed + 2**31) % 2**32) - 2**31            # size_t -> int32 narrowing (Sample.hpp:169)
            # ConstructSample (src/Sample.cpp:30-50): --bootstrap-count is the number of draws with --bin-reads;
            # the quirk without it passes the number of ITERATIONS as the count
            draws = (a.bootstrap_count if a.bin_reads else a.iters) if a.bootstrap_count > 0 else total
            w = ec_counts.astype(np.uint32)
            thetas, _ = core.bootstrap(w, seed, draws, 0, a.iters, prior, a.tol, a.max_iters, algo, prec)
            for row in thetas:
                sample.store_abundances(row)
    except MswError as ex:
        _say(a, f"Estimating relative abundances failed:\n  {ex}\nexiting\n")
        return 1
    names = grouping.get_names()
    mask = lik.groups_considered()
    est = [n for n, m in zip(names, mask) if m]
    zero = [n for n, m in zip(names, mask) if not m]
    if a.write_probs or a.print_probs:
        # Sample::write_probs (src/Sample.cpp:63-85): header ec_id + group names, one row per EC of exp(gamma)
        for dst in ([_open_out(core, path("probs.tsv"), a, "w")] if a.write_probs and a.prefix else []) + \
                   ([sys.stdout] if a.print_probs or (a.write_probs and not a.prefix) else []):
            write_probs(dst, est, zero if a.min_hits > 0 else [], core)
            if dst is not sys.stdout:
                dst.close()
    out = open(path("abundances.txt"), "w") if a.prefix else sys.stdout
    if a.run_rate:
        # experimental RATE / KLD (src/Sample.cpp:99-152, table written at src/mSWEEP.cpp:529-545)
        kld, rate = dirichlet_kld_rate(np.asarray(sample.get_abundances()) * total)
        sample._header(out)
        out.write("#c_id\tmean_theta\tRATE\tKLD\n")
        for n, t, r, k in zip(est, sample.get_abundances(), rate, kld):
            out.write(f"{n}\t{t:g}\t{r:g}\t{k:g}\n")
        for n in zero:
            out.write(f"{n}\t0\t0\t0\n")
        out.flush()
    elif a.min_hits > 0:
        sample.write_abundances2(est, zero, out)
    else:
        sample.write_abundances(est, out)
    if a.prefix:
        out.close()
    else:
        out.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
