"""--samples FILE: the manifest of a study -- one sample per line, `<prefix> TAB <alignment files> [TAB <FASTQ files>]`,
the lists comma separated -- and everything about it that is judged before a device is touched.  The
prefix means what -o means, the second column what --themisto means, the third what --extract-reads means for that
sample.  Empty lines and lines beginning with `#` are skipped.  msweep_amd/cpp/samples_manifest.hpp is the same parser
with the same messages for msweep_mini."""
from collections import namedtuple

Sample = namedtuple("Sample", "prefix files fastqs line")      # fastqs: None without a third column


class ManifestError(ValueError):
    """what the drivers print as `Parsing arguments failed:\\n  <message>\\nexiting\\n`"""


# the command line's own flags for what a manifest line gives, in the order they are named when they collide
CONFLICTS = ("--themisto", "--themisto-1", "--themisto-2", "-o", "--read-likelihood", "--print-probs", "--extract-reads")


def normal_path(p):
    """`p` without empty and `.` components, `..` resolved against the component before it: two spellings of one
    place compare equal (no look at the file system: the directories may not exist yet)"""
    parts = []
    for c in p.split("/"):
        if c in ("", "."):
            continue
        if c == ".." and parts and parts[-1] != "..":
            parts.pop()
        elif c == ".." and p.startswith("/"):
            continue
        else:
            parts.append(c)
    return ("/" if p.startswith("/") else "") + "/".join(parts)


def bin_dir(prefix):
    """where a sample's bins and extracted reads go (binning.bin_path): the prefix up to its last '/', or '.'"""
    s = prefix.rfind("/")
    return normal_path("." if s < 0 else prefix[:s] + "/")


def read_manifest(path):
    """the samples of the manifest, in its order"""
    try:
        with open(path, newline="\n") as f:      # (a line ends at "\n"; one "\r" in front of it is dropped)
            lines = f.read().split("\n")
    except OSError:
        raise ManifestError(f"cannot open the sample manifest {path}") from None
    out = []
    for n, line in enumerate(lines, 1):
        if line.endswith("\r"):
            line = line[:-1]
        if not line or line.startswith("#"):
            continue
        cols = line.split("\t")
        if not 2 <= len(cols) <= 3:
            raise ManifestError(f"{path}, line {n}: {len(cols)} columns (a sample is <prefix> TAB <alignment files> [TAB <FASTQ files>])")
        if not cols[0]:
            raise ManifestError(f"{path}, line {n}: empty output prefix")
        lists = [c.split(",") for c in cols[1:]]
        if any(not p for l in lists for p in l):
            raise ManifestError(f"{path}, line {n}: empty path in a list")
        out.append(Sample(cols[0], lists[0], lists[1] if len(lists) > 1 else None, n))
    if not out:
        raise ManifestError(f"the sample manifest {path} has no sample")
    return out


def check_samples(path, samples, bin_reads):
    """what makes two samples of one run collide, and the third column's conditions"""
    for s in samples[1:]:
        if (s.fastqs is None) != (samples[0].fastqs is None):
            raise ManifestError(f"{path}, line {s.line}: FASTQ files on some lines and not on others")
    if samples[0].fastqs is not None and not bin_reads:
        raise ManifestError(f"{path}: a FASTQ column needs --bin-reads")
    prefixes, dirs = {}, {}
    for s in samples:
        key = normal_path(s.prefix)
        if key in prefixes:
            raise ManifestError(f"{path}, line {s.line}: the output prefix {s.prefix} is that of line {prefixes[key]}")
        prefixes[key] = s.line
    if bin_reads:
        # the bins <dir>/<group>.bin and the extracted reads carry no prefix
        for s in samples:
            d = bin_dir(s.prefix)
            if d in dirs:
                raise ManifestError(f"{path}, line {s.line}: with --bin-reads the prefix {s.prefix} lies in the directory of "
                                    f"line {dirs[d]}: the bins would overwrite each other")
            dirs[d] = s.line


def parse_devices(text):
    """--devices d0[,d1,...]: one worker per entry, an entry may repeat"""
    parts = text.split(",")
    if not all(x.isascii() and x.isdigit() and len(x) <= 9 for x in parts):
        raise ManifestError(f"--devices: {text} is not a list of device indices")
    return [int(x) for x in parts]


def from_args(given, samples_path, devices, bin_reads):
    """The refusals of --samples / --devices in their order.  `given`: the flags of CONFLICTS that the command line holds.
    Returns (samples, device list or None)."""
    if samples_path is None:
        raise ManifestError("--devices needs --samples")
    for flag in CONFLICTS:
        if flag in given:
            raise ManifestError(f"--samples can't be used with {flag}")
    devs = parse_devices(devices) if devices is not None else None
    samples = read_manifest(samples_path)
    check_samples(samples_path, samples, bin_reads)
    return samples, devs
