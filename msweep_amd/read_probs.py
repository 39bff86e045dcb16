"""--write-read-probs / --probs-threshold: what the driver decides without a GPU -- the flags it refuses, in the words both
drivers print, and the header of `<prefix>_read_probs.tsv`.  The rows come from the device (Core.sparse_probs; DESIGN.md
7k).  msweep_amd/cpp/msweep_mini.cpp holds the same rules for the C++ driver (tests/test_read_probs_flags_cpu.py)."""
import math

DEFAULT_THRESHOLD = 0.001
PIECE = 256 << 20     # bytes of text per SparseProbs.pieces call


class ReadProbsError(ValueError):
    """what the drivers print as `Parsing arguments failed:\\n  <message>\\nexiting\\n`"""


def threshold_of(text):
    """the value of --probs-threshold as given on the command line: a number in (0, 1]"""
    try:      # (decimal text only, as the C++ driver's strtod is held to: no blanks, no '_', no hexadecimal)
        x = float(text) if text == text.strip() and "_" not in text else math.nan
    except ValueError:
        x = math.nan
    if not 0.0 < x <= 1.0:      # (a NaN compares false)
        raise ReadProbsError(f"--probs-threshold must be a probability in (0, 1] (got {text})")
    return x


def check_flags(write, threshold_text, prefix, samples, read_likelihood, no_fit_model, nested):
    """The refusals, in this order; returns the threshold.  prefix / samples: -o is given / --samples takes its place."""
    tau = DEFAULT_THRESHOLD if threshold_text is None else threshold_of(threshold_text)
    if threshold_text is not None and not write:
        raise ReadProbsError("--probs-threshold needs --write-read-probs")
    if not write:
        return tau
    if not prefix and not samples:
        raise ReadProbsError("--write-read-probs needs -o")
    for flag, on in (("--read-likelihood", read_likelihood), ("--no-fit-model", no_fit_model), ("--nested", nested)):
        if on:
            raise ReadProbsError(f"--write-read-probs can't be used with {flag}")
    return tau


def header(threshold, names):
    """the lines the host writes in front of the rows: the threshold, one line per ESTIMATED group (g = its row in the
    resident likelihood, the number the rows carry), the column names"""
    return ("#threshold\t%.17g\n" % threshold + "".join(f"#group\t{g}\t{n}\n" for g, n in enumerate(names))
            + "#read_id\tgroup\tprob\n").encode()
