#!/bin/bash
# Dev tool: build the library of another revision for same-box A/B, e.g.
#   scripts/build_variant.sh base HEAD~1   -> rnnt-speech-recognition_amd/lib/libwarprnnt_base.so
# and run anything with RNNT_LIBWARPRNNT=<that path> to load it instead of the product library.
# The revision is exported into a scratch directory and built there by its own build.py (its sources, its flags).
set -euo pipefail
[ $# -eq 2 ] || { echo "usage: $0 NAME REV" >&2; exit 2; }
NAME=$1
REV=$2
ROOT=$(cd "$(dirname "$0")/.." && pwd)
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
git -C "$ROOT" archive "$REV" | tar -x -C "$T"
python "$T/rnnt-speech-recognition_amd/build.py" >/dev/null
OUT=$ROOT/rnnt-speech-recognition_amd/lib/libwarprnnt_$NAME.so
mkdir -p "$(dirname "$OUT")"
cp "$T/rnnt-speech-recognition_amd/lib/libwarprnnt.so" "$OUT"
echo "$OUT"
