"""
Register / scratch / LDS figures of every kernel of the given csrc translation units, one line per kernel, from hipcc's
-Rpass-analysis=kernel-resource-usage remarks with the flags of pokerrl_amd/build.py (cross-compiles without a GPU):

    python scripts/kernel_resource_table.py prl_st_spec9.hip prl_st_spec33.hip prl_fhp_kernels.hip > listing.txt
    python scripts/kernel_resource_table.py --raw remarks_of_one_unit.txt ...      # remarks already collected (a file per unit)

Two listings made before and after a change to shared kernel source are compared with diff: equal lines = the same allocation.
"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIELDS = (("sgpr", r"TotalSGPRs: (\d+)"), ("vgpr", r" VGPRs: (\d+)"), ("agpr", r"AGPRs: (\d+)"), ("scratch_B", r"ScratchSize \[bytes/lane\]: (\d+)"),
          ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"), ("sgpr_spill", r"SGPRs Spill: (\d+)"), ("vgpr_spill", r"VGPRs Spill: (\d+)"),
          ("lds_B", r"LDS Size \[bytes/block\]: (\d+)"))


def table(unit, remarks):
    rows = []
    for block in re.split(r"remark: Function Name: ", remarks)[1:]:
        name = block.split(" ", 1)[0].split("\n", 1)[0]
        vals = []
        for key, pat in FIELDS:
            m = re.search(pat, block)
            vals.append("%s %s" % (key, m.group(1) if m else "-"))
        rows.append("%s  %s  %s" % (unit, name, "  ".join(vals)))
    return sorted(rows)


def main():
    args = sys.argv[1:]
    raw = args and args[0] == "--raw"
    for a in args[1:] if raw else args:
        if raw:
            unit, text = os.path.basename(a).rsplit(".", 1)[0], open(a).read()
        else:
            from pokerrl_amd import build as B
            cmd = [B.HIPCC] + B.COMMON + B.DEVICE + ["-Rpass-analysis=kernel-resource-usage", "-x", "hip", "-c", os.path.join(B.CSRC, a), "-o", os.devnull]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
            if p.returncode != 0:
                sys.exit(p.stdout.decode(errors="replace"))
            unit, text = a.rsplit(".", 1)[0], p.stdout.decode(errors="replace")
        print("\n".join(table(unit, text)))


if __name__ == "__main__":
    main()
