"""The compiler's resource report of kernels.hip, one commit against another (no GPU needed):

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -Rpass-analysis=kernel-resource-usage -c kernels.hip -o /dev/null 2> report.txt
    python tools/kernel_resources.py parent_report.txt this_report.txt

Prints every kernel of the first report whose VGPRs, AGPRs, scratch, occupancy or LDS differ in the second, then the kernels only the
second has, with their registers, scratch and occupancy.  Kernels are matched by their mangled names; a post kernel that gained the
defaulted alpha-source template argument (a trailing `h` = unsigned char in front of the closing E) is matched with its old name, and so is one that gained the defaulted dither
argument (a trailing `Lb0E`)."""
import re
import sys

FIELDS = ("VGPRs", "AGPRs", "ScratchSize", "Occupancy", "LDS")


def parse(path):
    d, cur = {}, None
    for line in open(path):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            d[cur] = {}
            continue
        m = re.search(r"remark: [^:]*?(VGPRs|AGPRs|SGPRs|ScratchSize|Occupancy|LDS Size)[^:]*: (\d+)", line)
        if m and cur and m.group(1).split()[0] not in d[cur]:
            d[cur][m.group(1).split()[0]] = int(m.group(2))
    return d


def parent_name(n):
    # a post kernel that gained the defaulted dither template argument (a trailing `Lb0E` = false) is matched with its old name
    if re.match(r"_ZN3rsr\d+postproc_tiles\w*I", n) and n.endswith("Lb0EEEvNS_8PostArgsE"):
        return n[:-len("Lb0EEEvNS_8PostArgsE")] + "EEvNS_8PostArgsE"
    if re.match(r"_ZN3rsr(14postproc_tiles|18postproc_tiles_box|19postproc_tiles_area)I", n) and n.endswith("hEEvNS_8PostArgsE"):
        return n[:-len("hEEvNS_8PostArgsE")] + "EEvNS_8PostArgsE"
    return n


def main():
    a, b = parse(sys.argv[1]), parse(sys.argv[2])
    bn = {}
    for k, v in b.items():
        bn[parent_name(k) if parent_name(k) in a and parent_name(k) not in b else k] = v
    print("existing kernels of kernels.hip, parent against this commit: %d" % len(a))
    changed = 0
    for k in sorted(a):
        if k not in bn:
            print("  MISSING %s" % k)
            changed += 1
        elif any(a[k].get(f) != bn[k].get(f) for f in FIELDS):
            print("  CHANGED %s: %s -> %s" % (k, a[k], bn[k]))
            changed += 1
    print("  kernels whose VGPRs / AGPRs / scratch / occupancy / LDS differ: %d" % changed)
    new = [k for k in sorted(bn) if k not in a]
    print("new instantiations: %d" % len(new))
    print("  %-72s %5s %5s %7s %4s" % ("kernel (mangled)", "VGPR", "SGPR", "scratch", "occ"))
    for k in new:
        v = bn[k]
        print("  %-72s %5d %5d %7d %4d" % (k, v["VGPRs"], v.get("SGPRs", -1), v["ScratchSize"], v["Occupancy"]))
    print("  new instantiations with scratch: %d" % sum(1 for k in new if bn[k]["ScratchSize"]))


if __name__ == "__main__":
    main()
