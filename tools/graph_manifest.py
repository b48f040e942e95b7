#!/usr/bin/env python3
"""Record tests/golden/graph_manifest.json: every form of tests/graph_forms.py run on the engine as it is NOW.  The manifest exists to pin the graph
code across a restructuring, so it is recorded at the commit BEFORE the restructuring (the hash it stores) and not regenerated from the new code;
tests/test_graph_manifest_gpu.py compares the current engine with it field by field.

    python tools/graph_manifest.py [--out tests/golden/graph_manifest.json] [--only NAME ...]

Every form must give at least one detection per image in every forward (the detection hash pins nothing otherwise): the tool fails if one does not.
A form's hash is kept only if two runs of its canvas sequence agree; forms that lose theirs are listed under "hash_dropped"."""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "instancesegmentation-jittor_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


class StderrToFile:
    """file descriptor 2 into a temporary file between begin() and end()"""

    def begin(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)

    def end(self):
        sys.stderr.flush()
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        text = self.tmp.read().decode()
        self.tmp.close()
        return text


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "graph_manifest.json"))
    ap.add_argument("--commit", default=None, help="the commit the engine was built from (default: git rev-parse HEAD)")
    ap.add_argument("--only", nargs="*", default=None)
    args = ap.parse_args()
    import graph_forms as gf
    from isegmi import _ffi
    _ffi.lib()
    assert _ffi.device_count() >= 1, "no HIP device"
    _ffi.set_device(0)
    commit = args.commit or subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"]).decode().strip()
    cap = StderrToFile()
    forms, dropped, empty = {}, [], []
    for form in gf.FORMS:
        if args.only and form["name"] not in args.only:
            continue
        rec = gf.run_form(form, cap.begin, cap.end)
        if any(c < 1 for step in rec["counts"] for c in step):
            empty.append(form["name"])
        if rec["hash"] != rec.pop("hash_repeat"):
            dropped.append(form["name"])
            del rec["hash"]
        forms[form["name"]] = rec
        print("%-36s counts %s  conv launches %d  marks %s" % (form["name"], rec["counts"], rec["conv_stats"]["launches"], rec["marks"][0]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(gf.pack(commit, dropped, forms))
    print("wrote %s (%d forms, %d without a hash) at %s" % (args.out, len(forms), len(dropped), commit))
    if empty:
        sys.exit("forms with an image without detections: " + ", ".join(empty))


if __name__ == "__main__":
    main()
