"""rocprofv3 kernel_trace.csv -> one line per launch in start order: grid (threads), workgroup, LDS, kernel name."""
import csv
import glob
import os
import sys


def main(d, out):
    tr = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = sorted(csv.DictReader(open(tr)), key=lambda r: (int(r["Start_Timestamp"]), int(r.get("Dispatch_Id", 0))))
    with open(out, "w") as f:
        for r in rows:
            f.write("grid %8sx%sx%s wg %5sx%sx%s lds %6s  %s\n" % (
                r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"], r["Workgroup_Size_X"], r["Workgroup_Size_Y"],
                r["Workgroup_Size_Z"], r.get("LDS_Block_Size", r.get("Group_Segment_Size", "?")), r["Kernel_Name"]))
    print("launches", len(rows), "columns", list(rows[0].keys()))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
