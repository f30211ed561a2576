from bayesianinferencedl_amd.deep_learning.dl_model import (ResBnFcModel, History, load_dataset_avg_rom, lr_schedule, lr_schedule_pre,  # noqa: F401
                                                            res_bn_fc_model, train_error_model)
