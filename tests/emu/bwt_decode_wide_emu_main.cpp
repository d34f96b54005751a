// TEST INFRASTRUCTURE -- BWT streams of the program at args[0] 5 .. 11 back into their blocks
// (zpaq_amd/csrc/device/bwt_decode_wide_kernel.h: the eight kernels over 8-byte nodes, the small decoder's count among them) on
// the host-side wavefront emulator.  The driver, its command line and what it prints: bwt_decode_emu_driver.h.
#include "bwt_decode_emu_driver.h"

int main(int argc, char** argv) { return BwtEmu<true>::main(argc, argv); }
