// sweep_wide.hip -- the sweeps over wide (8-byte) records: every k_passA / k_passB instantiation of that encoding and their launches.
#include "sweep_launch.hpp"

MSW_SWEEP_UNIT(wide, ENC == kEncWide)
