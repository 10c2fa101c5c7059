#!/bin/bash
# parity of the twelve-wave kernel on 8 / 16 / 13 / 5 streams and its kernel rate beside the eight-wave form, alternating, in one call: bash tools/x3_ab.sh [rounds]
cd "$(dirname "$0")/.."
timeout -k 10 300 python tests/tools/x3_check.py 6 2048 "${1:-3}"
