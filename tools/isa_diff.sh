#!/bin/bash
# Proves that a kernel refactor is a no-op: the device assembly of every shipped source, working tree against a git revision.
#   tools/isa_diff.sh REV [file.hip ...]   -> "identical" or the number of differing lines per file; exits non-zero if any differs
# REV's unimatch_amd/csrc + include are unpacked (git archive) into a temporary directory; each file of build.py's SOURCES (or the
# ones named) is compiled from both trees with the build's own flags (FLAGS + EXTRA_FLAGS per file) plus --cuda-device-only -S
# -fuse-cuid=none (without it two compilations of one source differ in their __hip_cuid_<hash> symbol).  ISA_DIFF_SIDE=host compares
# the host halves instead (--cuda-host-only).  A text comparison only.  ISA_DIFF_KEEP=1 keeps the .s files and prints where.
REV=${1:?usage: tools/isa_diff.sh REV [file.hip ...]}; shift
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
TMP=$(mktemp -d) || exit 2
[ -n "${ISA_DIFF_KEEP:-}" ] && echo "assembly kept in $TMP" || trap 'rm -rf "$TMP"' EXIT
mkdir "$TMP/old" "$TMP/new"
git -C "$ROOT" archive "$REV" unimatch_amd/csrc include | tar -x -C "$TMP/old" || exit 2
files=${*:-$(cd "$ROOT" && python -c "from unimatch_amd.build import SOURCES; print(' '.join(SOURCES))")}
side=--cuda-${ISA_DIFF_SIDE:-device}-only
bad=0
for f in $files; do
  flags=$(cd "$ROOT" && python -c "from unimatch_amd.build import FLAGS, EXTRA_FLAGS; print(' '.join(FLAGS + EXTRA_FLAGS.get('$f', [])))")
  for side_dir in "$TMP/old" "$ROOT"; do
    out="$TMP/new/$f.s"; [ "$side_dir" = "$ROOT" ] || out="$TMP/old/$f.s"
    (cd "$side_dir/unimatch_amd/csrc" && /opt/rocm/bin/hipcc $flags $side -S -fuse-cuid=none -w -o "$out" "$f") &
  done
  wait
  if [ ! -s "$TMP/old/$f.s" ] || [ ! -s "$TMP/new/$f.s" ]; then echo "$f: did not compile"; bad=1; continue; fi
  n=$(diff "$TMP/old/$f.s" "$TMP/new/$f.s" | grep -c '^[<>]')
  if [ "$n" = 0 ]; then echo "$f: identical"; else echo "$f: $n lines differ"; bad=1; fi
done
exit $bad
