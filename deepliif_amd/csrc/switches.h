// switches.h -- the ids of the runtime switches (include/deepliif_hip.h, "Runtime switches"): ONE list for the code that reads a switch (common.h:
// dl_switch(id)) and for the table that holds their names and load-time values (error.cpp: g_sw_names, in this order).
#pragma once
enum { DL_SW_CONV_S2F = 0, DL_SW_CONV_S2FX3, DL_SW_CONV_W4X3, DL_SW_PACK_TILED, DL_SW_NO_X3_GLDS, DL_SW_NO_WGRAD_C4, DL_SW_NO_C4_X3, DL_SW_CONV_S2D, DL_SW_CONV_DOT, DL_SW_COUNT };
