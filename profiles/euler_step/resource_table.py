"""-Rpass-analysis=kernel-resource-usage remarks -> one row per kernel instance, and the comparison of two tables.

  resource_table.py table UNIT.remarks [...] > table.tsv     (the compiler's stderr of each unit, saved to a file)
  resource_table.py compare parent.tsv branch.tsv            (one line: matched and differing instances)
"""
import re
import sys

FIELDS = ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]")
ROW = re.compile(r"remark:\s+(.*?): (\S+) \[-Rpass-analysis")


def table(paths):
    print("\t".join(("unit", "instance") + FIELDS))
    for path in paths:
        unit, name, row = path.rsplit("/", 1)[-1].split(".")[0], None, {}
        for line in open(path):
            m = ROW.search(line)
            if not m:
                continue
            if m.group(1) == "Function Name":
                name, row = m.group(2), {}
            elif name:
                row[m.group(1)] = m.group(2)
                if m.group(1) == FIELDS[-1]:   # the last remark of an instance
                    print("\t".join([unit, name] + [row[f] for f in FIELDS]))
                    name = None


def compare(a, b):
    def load(p):
        return {tuple(r[:2]): r[2:] for r in (l.rstrip("\n").split("\t") for l in list(open(p))[1:])}
    ta, tb = load(a), load(b)
    both = [k for k in ta if k in tb]
    differ = [k for k in both if ta[k] != tb[k]]
    print(f"{len(ta)} parent instances, {len(tb)} branch instances, {len(both)} matched by mangled name, "
          f"{len(both) - len(differ)} equal in all five fields, {len(differ)} differing, "
          f"{len(ta) - len(both)} only in the parent, {len(tb) - len(both)} only in the branch")
    for k in differ:
        print("DIFF", *k, ta[k], tb[k])
    return 1 if differ or len(both) != len(ta) or len(both) != len(tb) else 0


if __name__ == "__main__":
    sys.exit(table(sys.argv[2:]) if sys.argv[1] == "table" else compare(*sys.argv[2:4]))
