#!/usr/bin/env python3
"""Command-line driver with the job of the reference's ``h5_to_ply.py``: every room of an HDF5 room file as an ASCII PLY cloud.

    python h5_to_ply.py data/s3dis_area5.h5 --rgb                        # scan colours               -> data/rgb/<room>.ply
    python h5_to_ply.py data/s3dis_area5.h5 --seg                        # instances, largest first   -> data/gt/<room>.ply
    python h5_to_ply.py data/s3dis_area5.h5 --cls --class-table s3dis.txt   # class colours           -> data/class/<room>.ply
    python h5_to_ply.py data/s3dis_area5.h5 --target 44 --class-table s3dis.txt   # the legend of room 44: rank, class, colour
    python h5_to_ply.py rooms.h5 --seg --resolution 0.2 --out clouds/

All rooms go through one batched device pass (equalisation, colours, vertex lines: learn_region_grow_amd.h5_to_ply).  The class names and
colours are read from --class-table (lines ``id name r g b``); the matplotlib legend window of --target is a list of printed lines here.
"""
import sys

from learn_region_grow_amd.h5_to_ply import main

if __name__ == '__main__':
    sys.exit(main())
