#!/usr/bin/env python3
"""Command-line driver with the job of the reference's ``examine_h5.py``: the datasets of an HDF5 file, one line each as h5py prints
them (``<HDF5 dataset "count_room": shape (312,), type "<i4">``) and one with their minimum, mean and maximum.  Host only (h5lite).

    python examine_h5.py data/scannet.h5
"""
import sys

from learn_region_grow_amd.h5_to_ply import examine_main

if __name__ == '__main__':
    sys.exit(examine_main())
