"""Group indicators (`-i` file): mirror of mSWEEP::Reference / Grouping (include/Reference.hpp:53-94,
include/Grouping.hpp:52-98): one line per reference sequence, one grouping per tab-separated column, group
ids in order of first appearance, sizes = sequences per group.  read_references gives every column (the
drivers run the estimation once per column, src/mSWEEP.cpp:282), read_reference one of them."""
import numpy as np


class Grouping:
    def __init__(self, indicators):
        self.name_to_id = {}
        self.names = []
        sizes = []
        ids = np.empty(len(indicators), np.uint32)
        for i, name in enumerate(indicators):       # AdaptiveGrouping::add_sequence (:75-80)
            gid = self.name_to_id.get(name)
            if gid is None:
                gid = len(self.names)
                self.name_to_id[name] = gid
                self.names.append(name)
                sizes.append(0)
            sizes[gid] += 1
            ids[i] = gid
        self.sizes = np.array(sizes, np.uint64)
        self.group_indicators = ids

    def get_n_groups(self):
        return len(self.names)

    def get_names(self):
        return self.names

    def get_sizes(self):
        return self.sizes

    def max_group_size(self):
        return int(self.sizes.max())


def _split(line, delimiter):
    """the fields of a line as repeated std::getline(stream, field, delimiter) yields them (include/Reference.hpp:74):
    an empty field between two delimiters is a field and a trailing delimiter adds none.  An empty line stays one
    empty field -- the group named "" it has always been in a single-column file"""
    parts = line.split(delimiter)
    if len(parts) > 1 and parts[-1] == "":
        parts.pop()
    return parts


def read_references(stream, delimiter="\t"):
    """ConstructAdaptiveReference (src/Reference.cpp:31-56) for every column: a list of Grouping, one per column of
    the first line.  A line with another number of fields is refused (the reference would end up with columns of
    different lengths)."""
    rows = [_split(ln.rstrip("\n"), delimiter) for ln in stream]
    if not rows:
        raise RuntimeError("The grouping contains 0 reference sequences")
    m = len(rows[0])
    for k, r in enumerate(rows):
        if len(r) != m:
            raise RuntimeError(f"The grouping has {len(r)} columns on line {k + 1}, {m} on line 1")
    return [Grouping([r[c] for r in rows]) for c in range(m)]


def output_path(prefix, index, n_groupings, name):
    """The file of an output of grouping `index` (src/OutfileDesignator.cpp:64-74,116-123): `<prefix>_<name>` for a
    single grouping, `<prefix>_<index>_<name>` when the -i file has several; without a prefix the bare name (the
    likelihood files: everything else goes to stdout then)."""
    if not prefix:
        return name
    return f"{prefix}_{index}_{name}" if n_groupings > 1 else f"{prefix}_{name}"


def read_reference(stream, delimiter="\t", column=0):
    """ConstructAdaptiveReference (src/Reference.cpp:31-56) for grouping `column`."""
    lines = [ln.rstrip("\n") for ln in stream]
    if not lines:
        raise RuntimeError("The grouping contains 0 reference sequences")
    return Grouping([ln.split(delimiter)[column] for ln in lines])
