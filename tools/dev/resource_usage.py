"""The compiler's resource usage per kernel, one sorted line each, from the log of a build with
CXXFLAGS='... -Rpass-analysis=kernel-resource-usage' -- two such listings are compared with diff (profiles/report_refactor_resources.txt).

    make -C turbomesh_amd/csrc CXXFLAGS="-O3 -std=c++17 -fPIC -ffp-contract=off -Rpass-analysis=kernel-resource-usage" 2> build.log
    python tools/dev/resource_usage.py < build.log > usage.txt"""
import re
import sys

FIELDS = [("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("TotalSGPRs", "sgpr"), ("ScratchSize [bytes/lane]", "scratch"), ("LDS Size [bytes/block]", "lds"),
          ("Occupancy [waves/SIMD]", "occupancy")]
LINE = re.compile(r"^(\S+?):\d+:\d+: remark:\s+(.*?): (\S+) \[-Rpass-analysis=kernel-resource-usage\]")


def main():
    kernels, name = {}, None
    for line in sys.stdin:
        m = LINE.match(line)
        if not m:
            continue
        source, key, value = m.groups()
        if key == "Function Name":
            name = f"{source} {value}"
            kernels[name] = {}
        elif name is not None:
            kernels[name][key] = value
    for name in sorted(kernels):
        print(name, " ".join(f"{short}={kernels[name].get(key, '?')}" for key, short in FIELDS))


if __name__ == "__main__":
    main()
