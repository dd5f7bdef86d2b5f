"""One test case per kernel in prims.o (the assembly's scan, sort and ordering primitives): kernel, as the demangler spells it
inside namespace ibh, -> the test in tests/test_gpu_prims.py that launches it and compares its result with an exact reference.
test_every_prims_kernel_is_exercised (tests/test_capi_symbols.py) asserts that the kernels built and this table are the same set."""

CASES = {
    "scan_chained<unsigned int>": "test_scan_exact",
    "scan_chained<unsigned char>": "test_scan_exact",
    "s3_tile_sums": "test_scan3_exact",
    "s3_sums_inplace": "test_scan3_exact",
    "s3_tile_apply": "test_scan3_exact",
    "rs_hist": "test_radix_sort_exact",
    "rs_scatter": "test_radix_sort_exact",
    "oa_tiles": "test_order_piece_size_classes",
    "oa_tile_prefix": "test_order_piece_size_classes",
    "oa_cut_flags": "test_order_piece_size_classes",
    "oa_work_list": "test_order_piece_size_classes",
    "oa_work_classify": "test_order_piece_size_classes",
    "oa_chunk_sort<2048, 1, 256>": "test_order_piece_size_classes",
    "oa_chunk_sort<4096, 2048, 512>": "test_order_piece_size_classes",
    "oa_chunk_sort<8192, 4096, 1024>": "test_order_piece_size_classes",
}
