// sweep_index.hip -- the sweeps over index records (the hybrid area) and value records: every k_passA / k_passB instantiation of
// those encodings and their launches.
#include "sweep_launch.hpp"

MSW_SWEEP_UNIT(index, ENC == kEncIndex || ENC == kEncValue)
