#!/bin/bash
# A/B of the shared-source forward: fwd_group = 0 / 2 / 4 receivers per group
for w in ${WORKLOADS:-chignolin dipeptide protein2000}; do
  python tools/kbench.py $w --option fwd_group=0 2>/dev/null | head -2 | tr '\n' ' '; echo
  for g in 2 4; do
    echo -n "[group=$g] "; python tools/kbench.py $w --option fwd_group=$g 2>/dev/null | sed -n 2,2p
  done
done
