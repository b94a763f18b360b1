#!/bin/bash
# Verification build of `lit`'s whole-bundle shadow decisions (rt_core.h: bundle_decide): compiled with the hooks of
# tools/decide_check_hooks.h (-DMCRT_KERNEL_HOOKS) every record's rays are traced even when the bundle was decided, and a
# decision the traced rays contradict is printed and counted.  The product library contains none of this.  usage: tools/decide_check.sh build   (here, no GPU needed)
#                                            tools/decide_check.sh run [first_seed count]   (on the GPU box)
R=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}
if [ "$1" = build ]; then
  mkdir -p $R/variants
  cd $R && python3 -c "from minecraftskin_raytracer_amd.build import build
build(force=True, out='$R/variants/decide_check.so', extra_flags=['-I$R/tools', '-DMCRT_KERNEL_HOOKS=\"decide_check_hooks.h\"'])"
  exit $?
fi
first=${2:-900000}; count=${3:-2000}
export MCRT_LIB=$R/variants/decide_check.so MCRT_GRAPH=0
for mode in "" bundle wide; do
  timeout -k 10 900 python3 $R/tools/gpu_fuzz.py $first $count $mode 2>&1 | grep -a "DECIDE_CHECK\|fuzz:" | python3 -c "
import sys, re
tot = [0, 0, 0, 0]; bad = []
for line in sys.stdin:
    m = re.search(r'records: (\d+) undecided, (\d+) decided all-shadowed, (\d+) decided all-lit, (\d+) CONTRADICTED', line)
    if m: tot = [a + int(b) for a, b in zip(tot, m.groups())]
    elif 'decided' in line: bad.append(line.strip())
    elif line.startswith('fuzz:'): print(line.strip())
print('records: %d undecided, %d decided all-shadowed, %d decided all-lit, %d contradicted' % tuple(tot))
for b in bad[:20]: print(b)
sys.exit(1 if tot[3] else 0)" || exit 1
done
