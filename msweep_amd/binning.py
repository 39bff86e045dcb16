"""--bin-reads: the driver side of the mGEMS binning step (src/mSWEEP.cpp:437-469).  The bins themselves come from the
device (Core.bin_reads_aln: msweep_amd/csrc/bin_kernels.hpp); this module holds, one function each, what the drivers
decide around them: which groups are targets, the --min-abundance filter, the thresholds 1 - theta, where a bin is
written and how.  The native driver (msweep_amd/cpp/msweep_mini.cpp) makes the same choices and writes the same bytes.
--write-unassigned / --write-assignment-table (Core.assign_reads_aln: msweep_amd/csrc/assign_kernels.hpp)
add the file of the unassigned bin, the table's header and its rows per block.

mGEMS itself is not vendored by the reference (fetched at configure time), so the rule is restated from the mGEMS paper
(Maklin et al., Microbial Genomics 7:11, 2021); DESIGN.md marks it [UPSTREAM-UNVERIFIED]."""
import numpy as np


class BinningError(RuntimeError):
    """"Binning the reads failed" (src/mSWEEP.cpp:458-460)."""


def resolve_targets(estimated_names, target_groups=None):
    """Target names (src/mSWEEP.cpp:438-443): every estimated group in group order, or the --target-groups list in the
    order given (a name listed twice is binned once).  A name that is not an estimated group -- unknown, or pruned by
    --min-hits -- is refused."""
    if target_groups is None:
        return list(estimated_names)
    known = set(estimated_names)
    out = []
    for name in target_groups:
        if name not in known:
            raise BinningError(f"target group {name} is not among the estimated groups")
        if name not in out:
            out.append(name)
    return out


def filter_min_abundance(targets, estimated_names, abundances, min_abundance):
    """mGEMS::FilterTargetGroups (src/mSWEEP.cpp:444-446): drops a target whose abundance is below min_abundance;
    ties are kept."""
    theta = dict(zip(estimated_names, abundances))
    return [t for t in targets if not theta[t] < min_abundance]


def thresholds(target_rows, abundances):
    """t_k = 1 - theta_k: the reads of an EC go to bin k when gamma(g_k, j) >= log t_k."""
    theta = np.asarray(abundances, np.float64)
    return 1.0 - theta[np.asarray(target_rows, np.int64)]


def bin_path(prefix, name):
    """OutfileDesignator::bin (src/OutfileDesignator.cpp:80-93): `-o` up to its last '/', or '.', then /<name>.bin."""
    d = prefix[:prefix.rfind("/")] if "/" in prefix else "."
    return d + "/" + name + ".bin"


def extract_path(prefix, name, k):
    """--extract-reads: the reads of target group `name` from the k-th FASTQ file (k from 1), beside the bins:
    <dir>/<name>_<k>.fastq.  This project's own rule [UPSTREAM-UNVERIFIED]: mGEMS is not vendored by the reference."""
    return bin_path(prefix, name)[:-len(".bin")] + f"_{k}.fastq"


UNASSIGNED = "unassigned_reads"      # --write-unassigned: the bin of the reads no estimated group claims


def unassigned_path(prefix):
    """--write-unassigned: <dir>/unassigned_reads.bin, beside the bins (bin_path)."""
    return bin_path(prefix, UNASSIGNED)


def check_unassigned_name(estimated_names):
    """An estimated group literally named `unassigned_reads` would share the file of the unassigned bin: refused."""
    if UNASSIGNED in estimated_names:
        raise BinningError(f"a group is named {UNASSIGNED}, the name of the file --write-unassigned writes")


def all_thresholds(abundances):
    """t_g = 1 - theta_g for EVERY estimated group: what Core.assign_reads_aln judges every class against."""
    return 1.0 - np.asarray(abundances, np.float64)


def table_header(target_names):
    """first line of <prefix>_reads_to_groups.tsv: `#read_id`, then the target names in target order"""
    return ("\t".join(["#read_id"] + list(target_names)) + "\n").encode()


def table_block_rows(n_targets):
    """Rows per Core.assign_table_block call: 2^20, fewer when the worst-case text of a block (11 + 2 n_targets bytes per
    row) would exceed 256 MiB."""
    return max(1, min(1 << 20, (256 << 20) // (11 + 2 * int(n_targets))))


def format_ids(ids):
    """One decimal id per line, each line ending in '\\n' (mGEMS::WriteBin), formatted with array operations:
    10 M ids in well under a second."""
    v = np.asarray(ids, np.uint32).astype(np.uint64)
    if len(v) == 0:
        return b""
    nd = np.ones(len(v), np.int64)
    t = v // 10
    while True:
        nz = t > 0
        if not nz.any():
            break
        nd += nz
        t //= 10
    ends = np.cumsum(nd + 1)                      # one past each line's '\n'
    buf = np.empty(int(ends[-1]), np.uint8)
    buf[ends - 1] = ord("\n")
    pos = ends - 2                                # the last digit of each id
    for d in range(int(nd.max())):
        m = nd > d if d else slice(None)
        buf[pos[m] - d] = (v[m] % 10).astype(np.uint8) + ord("0")
        v[m] //= 10
    return buf.tobytes()


def write_bin(path, ids):
    with open(path, "wb") as f:
        f.write(format_ids(ids))
