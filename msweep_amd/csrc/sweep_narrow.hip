// sweep_narrow.hip -- the sweeps over narrow (4-byte offset) records: every k_passA / k_passB instantiation of that encoding,
// pass B's short-slice (RC = 8) ones included, and their launches.
#include "sweep_launch.hpp"

MSW_SWEEP_UNIT(narrow, ENC == kEncNarrow)
