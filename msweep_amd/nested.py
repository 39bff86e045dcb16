"""--nested: the K >= 2 columns of -i as ONE hierarchy, column 0 the coarsest.  A node is a list of group
names (g0, ..., g(d-1)), the root the empty list; its stem is the names joined by `_`.  Here is everything about the tree
that is judged before a device is touched, and the names of a node's files; msweep_amd/cpp/nested_tree.hpp is the same
for msweep_mini, with the same messages (tests/test_nested_flags_cpu.py holds them against each other)."""


class NestedError(ValueError):
    """what the drivers print as `Parsing arguments failed:\\n  <message>\\nexiting\\n`"""


# the flags --nested refuses, in the order they are named when several are given
CONFLICTS = ("--read-likelihood", "--no-fit-model", "--alphas", "--write-unassigned", "--write-assignment-table", "--print-probs")


def stem(names):
    return "_".join(names)


def show(names):
    """a label path as the messages print it"""
    return " > ".join(names) if names else "(root)"


def node_path(prefix, node_stem, name):
    """a node's output: `<prefix>[_<stem>]_<name>` -- the root's names are the single-column names; without a prefix the
    bare name, `<stem>_<name>` below the root (the likelihood files: everything else goes to stdout then)"""
    mid = node_stem + "_" if node_stem else ""
    return f"{prefix}_{mid}{name}" if prefix else mid + name


def bin_name(node_stem, group):
    """the file stem of a node's bin for `group`: `<group>` at the root, as without --nested, `<stem>_<group>` below"""
    return f"{node_stem}_{group}" if node_stem else group


def check_flags(given):
    """`given`: the flags of CONFLICTS that the command line holds"""
    for flag in CONFLICTS:
        if flag in given:
            raise NestedError(f"--nested can't be used with {flag}")


def check_tree(path, rows):
    """rows: the fields of every line of the -i file (all of one length).  One column, a group name with '/', and two
    distinct label paths -- of any depth, the root included -- whose stems are the same name are refused: stems name the
    nodes' files and, one level down, the bins."""
    K = len(rows[0])
    if K < 2:
        raise NestedError(f"--nested needs at least two columns in -i ({path} has {K})")
    seen = {"": ()}
    for r in rows:
        for d in range(1, K + 1):
            p = tuple(r[:d])
            if "/" in p[-1]:
                raise NestedError(f"{path}: the group name {p[-1]} contains '/' (--nested names files by group)")
            s = stem(p)
            first = seen.setdefault(s, p)
            if first != p:
                raise NestedError(f"{path}: the label paths {show(first)} and {show(p)} give the same name `{s}`")
