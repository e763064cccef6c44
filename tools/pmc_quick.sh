#!/bin/bash
# tools/pmc_quick.sh OUT [--script "SCRIPT ARGS"] GROUP ...: one rocprofv3 --kernel-trace --pmc pass per quoted counter group (tools/ab.py pmc)
python3 "$(dirname "$0")/ab.py" pmc "$@"
