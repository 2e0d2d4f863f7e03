"""What the probes read of a rocprofv3 --kernel-trace run (sample_probe.py, logp_probe.py, gae_probe.py)."""
import csv
import glob
import os


def kernel_times(trace_dir, name):
    """The durations in us, in start order, of the dispatches under trace_dir whose kernel name contains `name`."""
    files = sorted(glob.glob(os.path.join(trace_dir, '**', '*kernel_trace.csv'), recursive=True))
    if len(files) != 1:
        raise SystemExit(f'expected one *kernel_trace.csv under {trace_dir}, found {files}')
    rows = [r for r in csv.DictReader(open(files[0])) if name in r['Kernel_Name']]
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    return [(int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1000.0 for r in rows]
