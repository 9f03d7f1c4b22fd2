"""The dispatch-switch environments of the debug library (csrc/common.h rd_switch) that the conv parity tests are re-run under
(test_gpu_ops.py test_conv_kernels_under_forced_dispatch) and whose routes tests/golden/conv_routes.json pins on the CPU
(test_cpu_conv_routes.py): one list, so that the two cannot drift."""
ENVS = [
    {'RD_CONV_WS': '3', 'RD_CONV_WS_MIN2': '0', 'RD_CONV_NB1_BELOW': '0'},          # conv_ws_kernel: forward AND gradient launches
    {'RD_CONV_WS': '3', 'RD_CONV_WS_MIN2': '0', 'RD_CONV_NB1_BELOW': '0', 'RD_CONV_WS_FLAT': '0'},   # ... on 8 x 32 tiles only
    {'RD_CONV_WS': '3', 'RD_CONV_WS_MIN2': '1073741824', 'RD_CONV_NB1_BELOW': '0'},  # conv_ws_kernel forward, gradients on conv_pf_kernel (the round-3 default)
    {'RD_CONV_WS': '0', 'RD_CONV_PP_ALL': '1', 'RD_CONV_NB1_BELOW': '0'},           # conv_pp_kernel (LDS-staged epilogue) everywhere
    {'RD_CONV_PP_OFF': '1', 'RD_CONV_NB1_BELOW': '0'},                              # conv_pf_kernel with the register epilogues
    {'RD_CONV_PP_OFF': '1', 'RD_CONV_NB1_BELOW': '0', 'RD_CONV_FLAT_TILES': '0'},   # ... on 8 x 32 tiles only (default: 10 x 25 where more lanes are live)
    {'RD_CONV_PP_OFF': '1', 'RD_CONV_PF_LEAN_OFF': '1', 'RD_CONV_NB1_BELOW': '0'},  # conv_pf_kernel with the LDS-staged epilogue
    {'RD_CONV_NB1_BELOW': '100000'},                                                # 32-wide tiles for every 64-wide launch
    {'RD_SW_TPW': '5'},                                                             # conv_small_fwd_kernel: 5 tiles per workgroup (+ ghosts)
    {'RD_SW_TPW': '2'},                                                             # ... fewer tiles than register sets
    {'RD_SW_NWV': '4'},                                                             # ... two 256-thread workgroups per CU, two tile rows per wave (<= 16-channel inputs)
    {'RD_SW_NWV': '4', 'RD_SW_TPW': '5'},
    {'RD_SW_NWV': '8'},                                                             # ... one 512-thread workgroup per CU for every input width
    {'RD_CONV_SMALL_FWD': '0'},                                                      # conv_small_kernel for the forward launches
]
IDS = ['ws_fwd_bwd', 'ws_fwd_bwd_8x32', 'ws_fwd_pf_bwd', 'pp_staged', 'pf_lean', 'pf_lean_8x32', 'pf_staged', 'nb1_everywhere', 'small_fwd_tpw5', 'small_fwd_tpw2', 'small_fwd_nwv4', 'small_fwd_nwv4_tpw5', 'small_fwd_nwv8', 'small_fwd_off']
