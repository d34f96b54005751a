// TEST INFRASTRUCTURE -- BWT streams back into their blocks (zpaq_amd/csrc/device/bwt_decode_kernel.h: the six kernels over
// 4-byte nodes) on the host-side wavefront emulator.  The driver, its command line and what it prints: bwt_decode_emu_driver.h.
#include "bwt_decode_emu_driver.h"

int main(int argc, char** argv) { return BwtEmu<false>::main(argc, argv); }
