"""Writes tests/golden/structs.parquet and structs_expected.json: 120 rows of the struct tests'
shared table (tests/struct_tables.py: structs, a struct in a struct, a list of structs, a struct
of a list, a map, a required struct), two row groups, snappy, small pages.  Needs pyarrow; the
test that reads the file does not.  Run from anywhere: python tests/golden/make_structs_golden.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import struct_tables as ST  # noqa: E402


def main():
    rows = ST.rows(120, seed=17)
    data = ST.file_bytes(ST.table(rows), compression="snappy", data_page_size=300, write_batch_size=20,
                         row_group_size=60, write_statistics=False)
    with open(os.path.join(HERE, "structs.parquet"), "wb") as f:
        f.write(data)
    # rows as the tree's to_pylist gives them, in JSON's terms: strings as they are, a map as
    # a list of [key, value]
    as_json = json.loads(json.dumps(rows))
    with open(os.path.join(HERE, "structs_expected.json"), "w") as f:
        json.dump(as_json, f, indent=None, separators=(",", ":"))
        f.write("\n")
    print(len(data), "bytes,", len(rows), "rows")


if __name__ == "__main__":
    main()
